"""The invariant maps with kernels of their own on one MI355X: forward + backward of MaxFilteringInvariant, CanonizationInvariant,
PolynomialInvariant and ThirdOrderInvariant at the invariant ViT-H/14 hand-off shape (M = 64 x 257 rows, c = 160, R = 2560
references), in bf16 (autocast) and f32.

Arms, alternating in one process on the same seeded operands:
  engine  csrc/orbit_invariant.hip / csrc/poly_invariant.hip through the modules (d8_invariantization.ORBIT_HIP / POLY_HIP = True);
  stock   ORBIT_HIP / POLY_HIP = False: the reference's composition (expanded references / orbit, einsum, max / argmax + gather;
          for the polynomial maps one torch kernel per multiply, add and negate of the monomial table, then torch.cat).
Each window is `--window` iterations (MaxFiltering) or `--canon-window` iterations (Canonization: two row kernels of ~0.1 ms,
so a short window would time the host's launches) between one pair of HIP events; reported is the median over `--iters` windows
with minimum and maximum in milliseconds per iteration, the ratio stock / engine, and the peak allocation of one iteration of
each arm above what is resident before it.  MaxFiltering's engine arm also reports TFLOP/s on the 12-partial count (72 M R c
for forward + both gradients) with its fraction of the MFMA peak of the dtype (2500 TF bf16, 157.3 TF f32); Canonization has
no MFMA and no R: it reports the bytes its two kernels must move (read x, write out, read the cotangent, write dx) per second.
The polynomial maps use the Canonization window (two kernels of ~0.1 ms) and report the same compulsory bytes: x f32 read twice,
dx f32 written, out written and the cotangent read in the output dtype (P = 32 / 15 planes).  Under bf16 autocast both of their
arms see what the models give them: `_out_dtype=bfloat16` and a bf16 cotangent - the stock arm ignores the keyword, returns f32,
and the `.to(bfloat16)` that `invariant_proj` applies under autocast is part of its iteration.

    python tools/bench_invariants.py [--iters 10] [--window 3] [--canon-window 50] [--maps max_filtering,canonization,polynomial,third_order]
                                     [--out profiles/bench_invariants.txt] [--append]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import d8_invariantization as INV  # noqa: E402
from octic_vits_amd import functional as OF  # noqa: E402

PEAK_TF = {torch.bfloat16: 2500.0, torch.float32: 157.3}


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


POLY = {"polynomial": (INV.PolynomialInvariant, 32), "third_order": (INV.ThirdOrderInvariant, 15)}


def make_arm(mod, x, gout, c, dtype, hip, poly=False):
    def it():
        INV.ORBIT_HIP = INV.POLY_HIP = hip
        try:
            x.grad = None
            mod.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                y = mod(OF.Octic(x, c), _out_dtype=dtype).to(dtype) if poly else mod(OF.Octic(x, c))
            y.backward(gout)
            return y
        finally:
            INV.ORBIT_HIP = INV.POLY_HIP = True
    return it


def window_ms(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench(which, dtype, args, lines):
    B, T, c, R = args.batch, args.tokens, args.c, args.refs
    M = B * T
    torch.manual_seed(0)
    poly = which in POLY
    if poly:
        mod, width = POLY[which][0](8 * c), POLY[which][1] * c
    else:
        mod = (INV.MaxFilteringInvariant(8 * c, num_references=R) if which == "max_filtering" else INV.CanonizationInvariant(8 * c)).cuda()
        width = R if which == "max_filtering" else 8 * c
    x = torch.randn(B, T, 8 * c, device="cuda").requires_grad_()
    gout = torch.randn(B, T, width, device="cuda", dtype=dtype)
    arms = {"engine": make_arm(mod, x, gout, c, dtype, True, poly), "stock": make_arm(mod, x, gout, c, dtype, False, poly)}
    grads, peaks = {}, {}
    for name, it in arms.items():
        for _ in range(2):
            it()
        grads[name] = x.grad.detach().clone()
        peaks[name] = peak_mib(it)
    res = {name: [] for name in arms}
    window = args.window if which == "max_filtering" else args.canon_window
    for _ in range(args.iters):
        for name, it in arms.items():
            res[name].append(window_ms(it, window))
    e, s = _median(res["engine"]), _median(res["stock"])
    if which == "max_filtering":
        tf = 72.0 * M * R * c / (e * 1e-3) / 1e12
        shape = f"M {M} c {c} R {R}"
        rate = f"engine {tf:8.3f} TFLOP/s = {100 * tf / PEAK_TF[dtype]:.2f} % of the MFMA peak"
    elif poly:
        es = 2 if dtype == torch.bfloat16 else 4
        nbytes = M * c * (3 * 8 * 4 + 2 * POLY[which][1] * es)
        shape = f"M {M} c {c}"
        rate = f"engine kernels' {nbytes / 2 ** 20:.0f} MiB at {nbytes / (e * 1e-3) / 1e12:.2f} TB/s of the whole iteration"
    else:
        es = 2 if dtype == torch.bfloat16 else 4
        shape = f"M {M} c {c}"
        rate = f"engine kernels' {4 * M * 8 * c * es / 2 ** 20:.0f} MiB at {4 * M * 8 * c * es / (e * 1e-3) / 1e12:.2f} TB/s of the whole iteration"
    # the arms round differently, so a near tie may pick another group element in one of them (a different term of dx, or for
    # Canonization another signed copy of the row): reported is the share of dx entries further apart than tol max |dx|,
    # tol = 1e-3 in f32 and 2^-5 in bf16 (8 ulp of the dtype both arms round dx to)
    gmax = max(float(grads["stock"].abs().max()), 1e-30)
    tol = 2.0 ** -5 if dtype == torch.bfloat16 else 1e-3
    diff = float(((grads["engine"] - grads["stock"]).abs() > tol * gmax).double().mean())
    lines.append(f"  {which:13s} {str(dtype)[6:]:8s} {shape}   engine {e:8.3f} ms ({min(res['engine']):.3f}, {max(res['engine']):.3f}) "
                 f"peak {peaks['engine']:8.1f} MiB   stock {s:8.3f} ms ({min(res['stock']):.3f}, {max(res['stock']):.3f}) peak {peaks['stock']:8.1f} MiB"
                 f"   stock / engine {s / e:5.2f}   {rate}"
                 f"   dx entries apart by > {tol:.1e} max |dx|: {100 * diff:.3f} %")
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--canon-window", type=int, default=50)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--tokens", type=int, default=257)
    ap.add_argument("--c", type=int, default=160)
    ap.add_argument("--refs", type=int, default=2560)
    ap.add_argument("--maps", default="max_filtering,canonization,polynomial,third_order")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_invariants: needs a GPU (no CPU path)")
    lines = [f"bench_invariants: {torch.cuda.get_device_name(0)}, forward + backward through the modules, ms per iteration: median "
             f"(min, max) of {args.iters} windows of {args.window} (MaxFiltering) / {args.canon_window} (Canonization, Polynomial, ThirdOrder) "
             f"iterations, arms alternating"]
    for which in args.maps.split(","):
        for dtype in (torch.bfloat16, torch.float32):
            bench(which, dtype, args, lines)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
