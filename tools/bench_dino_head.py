"""The DINO / iBOT head of the DINOv2 step on one MI355X: ``ssl.DINOHead`` at the recipe's widths (1280 -> 2048 -> 2048 -> 256 ->
65 536 prototypes) under bf16 autocast, at the row counts of the 32-image step - the student's call (8 B local + 2 B global class
tokens + `upperbound` masked patch rows, forward + backward) and the teacher's (2 B + `upperbound`, forward under no_grad).

Arms, alternating in one process on the same parameters and rows:
  engine  ssl.DINO_HEAD_HIP on: csrc/dense_gemm.hip, csrc/dense_wgrad.hip, csrc/dino_norm.hip;
  stock   the switch off: nn.Linear / nn.GELU / F.normalize / weight_norm on the BLAS library and ATen.

EAGER ONLY, on the default stream, timed with one pair of HIP events around `--window` iterations.  A backward pass through a
DINOHead must never be captured in a hipGraph or run on a side stream: the module keeps the AccumulateGrad nodes of weight_g /
weight_v alive from its constructor on, stamped with the stream it was built on (NOTES 'DINO head'; the graph-captured ancestor of
this tool crashed on exactly that).  Eager times include the launches' host cost, which the step pays too.

Reported: per call and arm the median (min, max) over `--iters` windows in microseconds per iteration, and per kernel of the
engine arm (ops.KERNEL_TIMER, one extra untimed iteration) time, algorithmic bytes or FLOPs and the fraction of the 8.0 TB/s HBM
peak (row kernels, operand preparation) or of the 2.5 PFLOP/s dense bf16 MFMA peak (GEMMs); a launch shorter than 5 us is at
the resolution of an event pair and gets no rate.

    python tools/bench_dino_head.py [--images 32] [--iters 9] [--window 10] [--out profiles/bench_dino_head.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import functional as OF  # noqa: E402
from octic_vits_amd import ops  # noqa: E402
from octic_vits_amd import ssl as S  # noqa: E402

HBM_PEAK = 8.0e12
MFMA_PEAK_BF16 = 2.5e15
RESOLVED_US = 5.0          # a bracket shorter than this is a few event-pair overheads long: no rate is derived from it


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_arm(head, x, cot, engine, backward):
    def it():
        S.DINO_HEAD_HIP = engine
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                if not backward:
                    with torch.no_grad():
                        return head(x)
                for p in head.parameters():
                    p.grad = None
                x.grad = None
                y = head(x)
            y.backward(cot)
            return y
        finally:
            S.DINO_HEAD_HIP = True
    return it


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernel_lines(fn):
    ops.KERNEL_TIMER.enable()
    try:
        fn()
        agg = ops.KERNEL_TIMER._agg()
    finally:
        ops.KERNEL_TIMER.disable()
        ops.KERNEL_TIMER.records = []
    lines, total = [], 0.0
    for a in sorted(agg.values(), key=lambda a: -a["total_us"]):
        us = a["avg_us"]
        total += a["total_us"]
        if us < RESOLVED_US:
            rate = (f"{a['alg_bytes_per_launch'] / 1e6:9.2f} MB     launch-bound: at the resolution of an event pair, the rows sit in cache - "
                    f"no bandwidth figure")
        elif a["flops_per_launch"]:
            rate = f"{a['flops_per_launch'] / 1e9:9.2f} GFLOP  {a['flops_per_launch'] / max(us, 1e-3) / 1e6:7.1f} TFLOP/s = {100 * a['flops_per_launch'] / max(us, 1e-3) * 1e6 / MFMA_PEAK_BF16:5.1f} % of the bf16 MFMA peak"
        else:
            rate = f"{a['alg_bytes_per_launch'] / 1e6:9.2f} MB     {a['alg_bytes_per_launch'] / max(us, 1e-3) / 1e6:7.2f} TB/s    = {100 * a['alg_bytes_per_launch'] / max(us, 1e-3) * 1e6 / HBM_PEAK:5.1f} % of the HBM peak"
        lines.append(f"      {a['name']:44s} x{a['launches']}  {us:8.1f} us  {rate}")
    lines.append(f"      sum of the bracketed launches {total:.1f} us (casts, transposes and the copies of autograd are outside the brackets)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino_head: needs a GPU (no CPU path)")
    if args.iters < 7:
        raise SystemExit("bench_dino_head: at least 7 samples per arm")
    B = args.images
    upperbound = int(S.synthetic_multicrop_batch(B, "cuda", seed=5)["upperbound"])
    torch.manual_seed(0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        head = S.DINOHead(in_dim=1280, out_dim=65536, hidden_dim=2048, bottleneck_dim=256, nlayers=3).cuda()
    lines = [f"bench_dino_head: {torch.cuda.get_device_name(0)}, DINOHead 1280 -> 2048 -> 2048 -> 256 -> 65536, bf16 autocast, eager launches on "
             f"the default stream, HIP events around windows of {args.window} iterations, us per iteration: median (min, max) of "
             f"{args.iters} windows, arms alternating; {B} images per GPU, upperbound {upperbound}"]
    g = torch.Generator(device="cuda").manual_seed(1)
    for call, rows, backward in (("student, forward + backward", 8 * B + 2 * B + upperbound, True),
                                 ("teacher, forward under no_grad", 2 * B + upperbound, False)):
        x = torch.randn(rows, 1280, generator=g, device="cuda").requires_grad_(backward)
        cot = (torch.randn(rows, 65536, generator=g, device="cuda") / 65536).to(torch.bfloat16)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if not OF.dino_head_ok(head, x):
                raise SystemExit("bench_dino_head: the head does not take the engine path at these shapes")
        arms = {"engine": make_arm(head, x, cot, True, backward), "stock": make_arm(head, x, cot, False, backward)}
        outs = {}
        for name, it in arms.items():
            for _ in range(3):
                outs[name] = it().detach().float()
        torch.cuda.synchronize()
        res = {name: [] for name in arms}
        for _ in range(args.iters):
            for name in arms:
                res[name].append(window_us(arms[name], args.window))
        e, s = _median(res["engine"]), _median(res["stock"])
        diff = float((outs["engine"] - outs["stock"]).abs().max()) / float(outs["stock"].abs().max())
        lines.append(f"  {call}, {rows} rows:   engine {e:8.1f} ({min(res['engine']):.1f}, {max(res['engine']):.1f})   stock {s:8.1f} "
                     f"({min(res['stock']):.1f}, {max(res['stock']):.1f})   stock / engine {s / e:5.2f}   max |out diff| / max |out| {diff:.1e}")
        lines.append("    kernels of one engine iteration:")
        lines += kernel_lines(arms["engine"])
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
