"""Condense a rocprofv3 --kernel-trace --stats output directory into a small text summary (top kernels by
total time) suitable for committing under profiles/.
usage: rocprof_summary.py <rocprofv3 output dir> <summary.txt> [substring ...]
Every further argument is a substring of kernel names: the summary then ends with the calls and the total time of ALL kernels
whose name contains it (not only the top 60), or says that there is none."""
import csv
import glob
import sys

d, out, needles = sys.argv[1], sys.argv[2], sys.argv[3:]
files = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
if not files:
    sys.exit("no *kernel_stats.csv under " + d)
rows = []
for f in files:
    with open(f) as fh:
        rows += list(csv.DictReader(fh))
tot = sum(float(r["TotalDurationNs"]) for r in rows)
rows.sort(key=lambda r: -float(r["TotalDurationNs"]))
with open(out, "w") as fh:
    fh.write(f"# rocprofv3 --kernel-trace --stats summary ({len(rows)} kernels, total {tot/1e6:.2f} ms of GPU kernel time)\n")
    fh.write(f"{'calls':>7} {'total_ms':>10} {'avg_us':>10} {'pct':>6}  name\n")
    for r in rows[:60]:
        fh.write(f"{int(r['Calls']):7d} {float(r['TotalDurationNs'])/1e6:10.3f} {float(r['AverageNs'])/1e3:10.2f} "
                 f"{float(r['Percentage']):6.2f}  {r['Name'][:150]}\n")
    for needle in needles:
        hits = [r for r in rows if needle in r["Name"]]
        fh.write(f"# kernels whose name contains '{needle}': " + (f"{len(hits)} kernels, {sum(int(r['Calls']) for r in hits)} calls, "
                 f"{sum(float(r['TotalDurationNs']) for r in hits) / 1e6:.3f} ms\n" if hits else "none\n"))
        for r in hits[:12]:
            fh.write(f"#   {int(r['Calls']):7d} {float(r['TotalDurationNs'])/1e6:10.3f} ms  {r['Name'][:150]}\n")
print(open(out).read())
