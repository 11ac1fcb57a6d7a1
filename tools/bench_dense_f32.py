"""The float32 dense GEMMs (csrc/dense_f32.hip) on one MI355X against the BLAS library, ViT-H/14 at rows = 64 x 257 tokens.

  (a) launches: the four linear layers of a ViT-H/14 block (qkv 3840 x 1280, proj 1280 x 1280, fc1 5120 x 1280, fc2 1280 x 5120)
      in the three directions - NT forward with bias, NN input gradient, TN weight gradient - twelve launches.  Engine:
      ops.dense_f32_nt / _nn / _tn (the TN time includes its slab reduction launch).  Library: F.linear, g @ W, g.t() @ x on the
      same float32 tensors.  `--window` launches back to back between one HIP event pair, `--iters` windows, the two arms
      alternating window by window; median us per launch, achieved TFLOP/s for 2 M N K operations, and the share of the 157.3
      TFLOP/s f32 MFMA peak (256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz).  All twelve are compute-bound: the operands of the
      largest (0.46 GB) move in 58 us at the HBM peak against 1.4 ms of MFMA work.
  (b) block: one float32 ViT-H/14 Layer_scale_init_Block, forward + backward with every parameter gradient, no autocast -
      functional.DENSE_F32_HIP on (the whole block on the engine) against off (stock PyTorch ops, the attention core on the
      engine's float32 kernels in both arms), alternating, one iteration per event pair; per-kernel times of the engine arm
      (KERNEL_TIMER, a pass of its own).

    python tools/bench_dense_f32.py [--iters 10] [--window 3] [--out profiles/bench_dense_f32.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import functional as OF  # noqa: E402
from octic_vits_amd import _lib, ops, vit  # noqa: E402

F32_MFMA_PEAK = 157.3e12
LAYERS = {"qkv": (3840, 1280), "proj": (1280, 1280), "fc1": (5120, 1280), "fc2": (1280, 5120)}     # name -> (N, K)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(us):
    return {"median_us": round(_median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1), "n": len(us)}


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench_launches(args, dev):
    M = args.rows
    g = torch.Generator(device=dev).manual_seed(0)
    out = {"rows": M, "window": args.window,
           "what": "us per launch; engine / library windows alternate; TF = 2 M N K / time; peak = share of 157.3 TF f32 MFMA"}
    for name, (N, K) in LAYERS.items():
        x = torch.randn(M, K, generator=g, device=dev)
        gy = torch.randn(M, N, generator=g, device=dev)
        w = torch.randn(N, K, generator=g, device=dev) * K ** -0.5
        b = torch.randn(N, generator=g, device=dev)
        arms = {"nt": (lambda: ops.dense_f32_nt(x, w, b), lambda: F.linear(x, w, b)),
                "nn": (lambda: ops.dense_f32_nn(gy, w), lambda: gy @ w),
                "tn": (lambda: ops.dense_f32_tn(gy, x), lambda: gy.t() @ x)}
        flops = 2.0 * M * N * K
        for kind, (eng, lib) in arms.items():
            a, r = eng(), lib()
            rel = float((a - r).norm() / r.norm())
            for _ in range(args.warmup):
                _window(eng, args.window), _window(lib, args.window)
            se, sl = [], []
            for _ in range(args.iters):
                se.append(_window(eng, args.window))
                sl.append(_window(lib, args.window))
            e, l = _stats(se), _stats(sl)
            for st in (e, l):
                st["TF"] = round(flops / st["median_us"] / 1e6, 1)
                st["peak"] = round(flops / (st["median_us"] * 1e-6) / F32_MFMA_PEAK, 3)
            op = {"nt": _lib.DENSE_F32_NT, "nn": _lib.DENSE_F32_NN, "tn": _lib.DENSE_F32_TN}[kind]
            out[f"{name}_{kind}"] = {"N": N, "K": K, "plan": ops.dense_f32_plan(op, M, N, K), "engine": e, "library": l,
                                     "engine_over_library_time": round(e["median_us"] / l["median_us"], 3),
                                     "rel_l2_between_arms": float(f"{rel:.3g}")}
        del x, gy, w, b
    return out


def bench_block(args, dev):
    B, T, D = args.rows // args.tokens, args.tokens, 1280
    torch.manual_seed(0)
    blk = vit.Layer_scale_init_Block(D, 16, mlp_ratio=4.0, qkv_bias=True, init_values=1e-4).to(dev).train()
    params = list(blk.parameters())
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(B, T, D, generator=g, device=dev).requires_grad_(True)
    cot = torch.randn(B, T, D, generator=g, device=dev)

    def run(on):
        OF.DENSE_F32_HIP = on
        for p in params + [x]:
            p.grad = None
        blk(x).backward(cot)

    def timed(on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(on)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3

    try:
        for _ in range(args.warmup):
            timed(True), timed(False)
        run(True)
        ge = [p.grad.detach().clone() for p in params]
        run(False)
        agree = max(float((a - p.grad).norm() / p.grad.norm()) for a, p in zip(ge, params))
        samples = {"engine": [], "stock": []}
        for _ in range(args.iters):
            samples["engine"].append(timed(True))
            samples["stock"].append(timed(False))
        out = {"B": B, "tokens": T, "dim": D, "what": "us per forward + backward of one float32 block, one iteration per event pair",
               "arms": {k: _stats(v) for k, v in samples.items()}, "max_rel_l2_between_arms_param_grads": float(f"{agree:.3g}")}
        out["engine_over_stock_time"] = round(out["arms"]["engine"]["median_us"] / out["arms"]["stock"]["median_us"], 3)
        ops.KERNEL_TIMER.enable()
        for _ in range(3):
            run(True)
        out["engine_kernels"] = ops.KERNEL_TIMER.summary()
        ops.KERNEL_TIMER.disable()
    finally:
        OF.DENSE_F32_HIP = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=257)
    ap.add_argument("--rows", type=int, default=64 * 257)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense_f32: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "launches": bench_launches(args, dev), "block": bench_block(args, dev)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
