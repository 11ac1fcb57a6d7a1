"""The Sinkhorn-Knopp teacher targets of the DINO / iBOT terms on one MI355X: the row kernels of csrc/ssl_loss.hip
(ssl.FUSED_LOSS_ROWS = True: Q = E u v is never stored) against the stock-torch composition of the reference
(ssl.FUSED_LOSS_ROWS = False: exp, a transposed view, the total sum and three rounds of row and column normalisation of the f32
K x B matrix), on bf16 teacher logits at the two shapes of the recipe with K = 65 536 prototypes:

  ibot: 1 920 masked patch rows (iBOTPatchLoss.sinkhorn_knopp_teacher, with its count tensor)
  dino:    64 class-token rows  (DINOLoss.sinkhorn_knopp_teacher)

The arms alternate in one process, one call per HIP event pair, the same logits; min / median / max per arm.  Bytes: what the
fused algorithm needs - with n iterations 2 n + 2 reads of the logits (the row maxima, n prototype sums, n - 1 sample sums
and the two sweeps of the final pass, whose second sweep of a 128 KB row is counted although it can hit L2) and one f32 write -
over the fused arm's median, as a share of the 8 TB/s HBM peak; the composition is charged what it moves itself
(exp reads bf16 and writes f32, every division and the last multiplication read and write, every sum reads: 26 + 40 n bytes
per element) for the same figure.
Per-kernel times of the fused arm (KERNEL_TIMER) in a pass of their own.

    python tools/bench_sinkhorn.py [--iters 30] [--warmup 5] [--out profiles/bench_sinkhorn.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402
from octic_vits_amd import ssl as S  # noqa: E402

HBM_PEAK = 8.0e12                    # HBM3E spec of the MI355X, as in bench.py
BF = torch.bfloat16


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(us):
    return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": len(us)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def fused_bytes(rows, K, n_it, es=2):
    # 2 n + 2 sweeps of the logits, the f32 result, and the slab partials of every prototype sum written and read once
    return rows * K * ((2 * n_it + 2) * es + 4) + 2 * n_it * ops.lib().octic_sinkhorn_slabs(rows) * K * 4


def composition_bytes(rows, K, n_it, es=2):
    # exp: es + 4; total sum: 4; / total: 8; per iteration: row sum 4, two divisions 16, column sum 4, two divisions 16; * B: 8
    return rows * K * (es + 4 + 4 + 8 + n_it * 40 + 8)


def bench_shape(name, rows, K, args, dev):
    g = torch.Generator(device=dev).manual_seed(rows)
    # cosine logits of a weight-normed last layer lie in [-1, 1]: exp(x / 0.04) and its total stay finite in the composition
    x = (torch.randn(rows, K, generator=g, device=dev) * 0.2).clamp_(-1, 1).to(BF)
    if name == "ibot":
        mod, count = S.iBOTPatchLoss(K), torch.tensor([rows], device=dev)
        call = lambda: mod.sinkhorn_knopp_teacher(x, args.temp, count, n_iterations=args.n_iterations)
    else:
        mod = S.DINOLoss(K)
        call = lambda: mod.sinkhorn_knopp_teacher(x, args.temp, n_iterations=args.n_iterations)

    def arm(fused):
        def run():
            S.FUSED_LOSS_ROWS = fused
            try:
                return call()
            finally:
                S.FUSED_LOSS_ROWS = True
        return run

    arms = {"fused": arm(True), "composition": arm(False)}
    for _ in range(args.warmup):
        for fn in arms.values():
            _timed(fn)
    a, b = arms["fused"](), arms["composition"]()
    assert a.is_contiguous() and torch.isfinite(b).all()
    agree = float(((a - b).abs() / b.max(dim=1, keepdim=True).values).max())
    samples = {k: [] for k in arms}
    for _ in range(args.iters):                          # alternating: both arms see the same machine state
        for k, fn in arms.items():
            samples[k].append(_timed(fn))
    out = {"rows": rows, "K": K, "dtype": "bf16", "n_iterations": args.n_iterations,
           "what": "us per sinkhorn_knopp_teacher call, one call per event pair, arms alternating",
           "arms": {k: _stats(v) for k, v in samples.items()},
           "max_abs_diff_between_arms_over_row_max": float(f"{agree:.3e}")}
    for k, nbytes in (("fused", fused_bytes(rows, K, args.n_iterations)), ("composition", composition_bytes(rows, K, args.n_iterations))):
        st = out["arms"][k]
        st["alg_MB"] = round(nbytes / 1e6, 1)
        st["GBps"] = round(nbytes / st["median_us"] / 1e3, 1)
        st["share_of_hbm_peak"] = round(nbytes / (st["median_us"] * 1e-6) / HBM_PEAK, 3)
    out["composition_over_fused"] = round(out["arms"]["composition"]["median_us"] / out["arms"]["fused"]["median_us"], 3)
    ops.KERNEL_TIMER.enable()
    for _ in range(5):
        arms["fused"]()
    out["fused_kernels"] = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--K", type=int, default=65536)
    ap.add_argument("--ibot-rows", type=int, default=1920)
    ap.add_argument("--dino-rows", type=int, default=64)
    ap.add_argument("--temp", type=float, default=0.04)
    ap.add_argument("--n-iterations", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sinkhorn: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0),
           "ibot": bench_shape("ibot", args.ibot_rows, args.K, args, dev),
           "dino": bench_shape("dino", args.dino_rows, args.K, args, dev)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
