"""The SwiGLU FFN of DINOv2's ViT-g/14 on one MI355X: the gate kernels of csrc/swiglu.hip, and one FFN branch on the engine
against the stock-torch composition of the reference module (dinov2/layers/swiglu_ffn.py) under bf16 autocast, at
rows = 64 x 257 tokens, width 1536, hidden 4096.

  (a) kernels: swiglu_fwd / swiglu_bwd (with the column sums of w12's bias gradient and their reduction) alone, `--window`
      launches back to back between one HIP event pair, `--iters` windows; median time per launch, achieved GB/s against the bytes
      the algorithm needs (6 / 10 bytes per element of the hidden activation) and the share of the 8 TB/s HBM peak.  The 0.4 /
      0.67 GB working sets exceed every cache level.
  (b) branch: x + gamma * w3(silu(x1) * x2) of one layer, forward + backward with every parameter gradient -
      engine: vit.SwiGLUFFNFused.forward_fused (csrc/dense_gemm.hip, csrc/swiglu.hip, csrc/dense_wgrad.hip, the residual tail);
      stock:  F.linear, chunk, F.silu, mul, F.linear, the layer-scale multiply and the residual add on the same module's
              parameters under torch.autocast - what the reference runs.
      The arms alternate in one process, one iteration per event pair, the same inputs; per-kernel times of the engine arm
      (KERNEL_TIMER, a pass of its own).

    python tools/bench_swiglu.py [--iters 20] [--window 10] [--out profiles/bench_swiglu.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402
from octic_vits_amd import vit  # noqa: E402

HBM_PEAK = 8.0e12                    # HBM3E spec of the MI355X, as in bench.py
BF = torch.bfloat16


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(us):
    return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": len(us)}


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench_kernels(args, dev):
    rows, H = args.rows, args.hidden
    g = torch.Generator(device=dev).manual_seed(0)
    x12 = torch.randn(rows, 2 * H, generator=g, device=dev).to(BF)
    ga = torch.randn(rows, H, generator=g, device=dev).to(BF)
    arms = {"swiglu_fwd": (lambda: ops.swiglu_fwd(x12, H), rows * H * 6),
            "swiglu_bwd": (lambda: ops.swiglu_bwd(x12, ga, want_colsum=False), rows * H * 10),
            "swiglu_bwd_colsum": (lambda: ops.swiglu_bwd(x12, ga, want_colsum=True), rows * H * 10)}
    for fn, _ in arms.values():
        for _ in range(args.warmup):
            _window(fn, args.window)
    samples = {k: [] for k in arms}
    for _ in range(args.iters):
        for k, (fn, _) in arms.items():
            samples[k].append(_window(fn, args.window))
    out = {"rows": rows, "H": H, "window": args.window,
           "what": "us per launch, back-to-back launches per event pair; swiglu_bwd_colsum includes the slab reduction launch"}
    for k, (_, nbytes) in arms.items():
        st = _stats(samples[k])
        st["alg_MB"] = round(nbytes / 1e6, 1)
        st["GBps"] = round(nbytes / st["median_us"] / 1e3, 1)
        st["share_of_hbm_peak"] = round(nbytes / (st["median_us"] * 1e-6) / HBM_PEAK, 3)
        out[k] = st
    return out


def bench_branch(args, dev):
    rows, D = args.rows, args.dim
    B, T = rows // args.tokens, args.tokens
    torch.manual_seed(0)
    ffn = vit.SwiGLUFFNFused(D, 4 * D).to(dev)
    assert ffn.w3.in_features == args.hidden, (ffn.w3.in_features, args.hidden)
    gamma = torch.nn.Parameter(torch.full((D,), 0.5, device=dev))
    params = list(ffn.parameters()) + [gamma]
    g = torch.Generator(device=dev).manual_seed(1)
    y = torch.randn(B, T, D, generator=g, device=dev).to(BF).requires_grad_(True)
    xres = torch.randn(B, T, D, generator=g, device=dev).requires_grad_(True)
    cot = torch.randn(B, T, D, generator=g, device=dev)

    def clear():
        for p in params + [y, xres]:
            p.grad = None

    def engine():
        with torch.autocast("cuda", dtype=BF):
            out = ffn.forward_fused(y, xres, gamma, None, BF)
        out.backward(cot)

    def stock():
        with torch.autocast("cuda", dtype=BF):
            out = xres + gamma * ffn(y)
        out.backward(cot)

    def timed(fn):
        clear()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    for _ in range(args.warmup):
        timed(engine), timed(stock)
    clear()
    engine()
    ge = [p.grad.detach().float().clone() for p in params]
    clear()
    stock()
    agree = max(float((a - p.grad.float()).norm() / p.grad.float().norm()) for a, p in zip(ge, params))
    samples = {"engine": [], "stock": []}
    for _ in range(args.iters):                          # alternating: both arms see the same machine state
        samples["engine"].append(timed(engine))
        samples["stock"].append(timed(stock))
    out = {"rows": rows, "dim": D, "H": args.hidden, "what": "us per forward + backward of one FFN branch, one iteration per event pair",
           "arms": {k: _stats(v) for k, v in samples.items()},
           "max_rel_l2_between_arms_param_grads": round(agree, 4)}
    out["stock_over_engine"] = round(out["arms"]["stock"]["median_us"] / out["arms"]["engine"]["median_us"], 3)
    ops.KERNEL_TIMER.enable()
    for _ in range(5):
        clear()
        engine()
    out["engine_kernels"] = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--tokens", type=int, default=257)
    ap.add_argument("--rows", type=int, default=64 * 257)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swiglu: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "kernels": bench_kernels(args, dev), "branch": bench_branch(args, dev)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
