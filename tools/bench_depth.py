"""The linear depth head of the DINOv2 hub (octic_vits_amd/depth.py, csrc/depth.hip) on one MI355X at the hub's ViT-L/14 shape:
518 x 518 images -> 37 x 37 patches, the class and patch tokens of 4 blocks, D 1024, 256 bins, upsample 4 -> 148 x 148 maps.
Arms, on the same tensors and the same weights, float32, under torch.no_grad():

  engine : BNHead.forward_tokens on the two HIP kernels (logits at patch resolution, then resize + normalise + expectation)
  stock  : the same module with depth.DEPTH_HIP = False - the reference's composition: NCHW permute, cat with the class token,
           bilinear resize of the 8192-channel tensor (B x 8192 x 148 x 148 floats), 1x1 convolution, relu, normalisation, einsum

Two measurements: the head alone on random tokens, at the largest batch (up to --max-batch) whose stock arm fits the free device
memory, and backbone + head (depth.dinov2_vitl14_ld, random weights, whole_inference with the final rescale) at
--backbone-batch.  The arms alternate in one process; a sample is one HIP event pair around `reps` calls (so that the engine
arm's window is tens of milliseconds too), divided by reps; min / median / max per arm.  Then, in a pass of its own, the
engine's per-kernel times (KERNEL_TIMER: "depth_logits_kernel" brackets the class-token launch and the MFMA launch) with
each kernel's algorithmic bytes and FLOPs and its share of its bound: the larger of FLOPs over the 157.3 TF f32 MFMA peak and
bytes over the 8 TB/s HBM peak, over the kernel's time.

    python tools/bench_depth.py [--iters 7] [--warmup 2] [--out profiles/bench_depth.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import depth, ops  # noqa: E402

HBM_PEAK = 8.0e12                    # HBM3E spec of the MI355X, as in bench.py
F32_MFMA_PEAK = 157.3e12             # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "n": len(s)}


def _timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _alternate(arms, reps, warmup, iters):
    for _ in range(warmup):
        for k, fn in arms.items():
            _timed(fn, reps[k])
    samples = {k: [] for k in arms}
    for _ in range(iters):                                     # alternating: the arms see the same machine state
        for k, fn in arms.items():
            samples[k].append(_timed(fn, reps[k]))
    out = {k: dict(_stats(v), calls_per_sample=reps[k]) for k, v in samples.items()}
    return out, round(out["stock"]["median_ms"] / out["engine"]["median_ms"], 2)


def _stock(fn):
    def run():
        depth.DEPTH_HIP = False
        try:
            return fn()
        finally:
            depth.DEPTH_HIP = True
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--backbone-batch", type=int, default=8)
    ap.add_argument("--grid", type=int, default=37)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    g, D, layers, u = args.grid, args.D, args.layers, 4
    C, T, n = 2 * D * layers, 1 + g * g, g * g
    # what the stock arm holds per image: the per-layer resized maps, their concatenation, logits and normalised bins
    per_image = 4 * (u * g) ** 2 * (2 * C + 3 * 256) + 4 * 2 * C * n
    free, _ = torch.cuda.mem_get_info()
    B = max(1, min(args.max_batch, int(0.7 * free // per_image)))
    head = depth._linear_depth_head(D, layers).to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    outs = [torch.randn(B, T, D, generator=gen, device=dev) for _ in range(layers)]
    pairs = [(o[:, 1:], o[:, 0]) for o in outs]
    res = {"device": torch.cuda.get_device_name(0), "grid": [g, g], "D": D, "layers": layers, "bins": 256, "upsample": u,
           "what": "ms per call, float32, torch.no_grad(), arms alternating, one event pair per sample",
           "head_alone": {"batch": B, "stock_arm_bytes_per_image_estimate": per_image, "free_device_bytes": free}}
    with torch.no_grad():
        eng = lambda: head.forward_tokens(pairs, (g, g))  # noqa: E731
        stk = _stock(eng)
        assert head.kernels_take(pairs)
        a, b = eng(), stk()
        res["head_alone"]["max_abs_difference_of_the_arms"] = float((a - b).abs().max())
        res["head_alone"]["depth_range"] = [float(b.min()), float(b.max())]
        del a, b
        arms, ratio = _alternate({"engine": eng, "stock": stk}, {"engine": 20, "stock": 1}, args.warmup, args.iters)
        res["head_alone"]["arms"], res["head_alone"]["stock_over_engine"] = arms, ratio
        res["head_alone"]["flops_per_image"] = {"stock_conv_on_the_resized_tensor": 2.0 * C * 256 * (u * g) ** 2,
                                                "engine_logits_at_patch_resolution": 2.0 * (C // 2) * 256 * n + 2.0 * (C // 2) * 256}
        # per-kernel pass
        ops.KERNEL_TIMER.enable()
        for _ in range(5):
            eng()
        kernels = {}
        for name, k in sorted(ops.KERNEL_TIMER._agg().items(), key=lambda kv: -kv[1]["total_us"]):
            us = k["avg_us"]
            t_mfma, t_hbm = k["flops_per_launch"] / F32_MFMA_PEAK * 1e6, k["alg_bytes_per_launch"] / HBM_PEAK * 1e6
            kernels[name] = {"avg_us": round(us, 1), "alg_bytes": int(k["alg_bytes_per_launch"]), "flops": int(k["flops_per_launch"]),
                             "GBps": round(k["alg_bytes_per_launch"] / us / 1e3, 1) if us > 0 else None,
                             "share_of_hbm_peak": round(t_hbm / us, 4) if us > 0 else None,
                             "TFLOPs": round(k["flops_per_launch"] / us / 1e6, 1) if us > 0 else None,
                             "bound": "mfma" if t_mfma >= t_hbm else "hbm",
                             "share_of_bound": round(max(t_mfma, t_hbm) / us, 4) if us > 0 else None}
        ops.KERNEL_TIMER.disable()
        res["head_alone"]["engine_kernels"] = kernels
        del outs, pairs
        torch.cuda.empty_cache()

        # backbone + head
        Bb = args.backbone_batch
        model = depth.dinov2_vitl14_ld(layers=4).to(dev).eval()
        x = torch.randn(Bb, 3, 14 * g, 14 * g, generator=gen, device=dev)
        eng = lambda: model.whole_inference(x, None, True)  # noqa: E731
        stk = _stock(eng)
        a, b = eng(), stk()
        res["backbone_and_head"] = {"model": "dinov2_vitl14_ld(layers=4), random weights, float32 eager", "batch": Bb,
                                    "image": [14 * g, 14 * g], "max_abs_difference_of_the_arms": float((a - b).abs().max())}
        del a, b
        arms, ratio = _alternate({"engine": eng, "stock": stk}, {"engine": 1, "stock": 1}, args.warmup, args.iters)
        res["backbone_and_head"]["arms"], res["backbone_and_head"]["stock_over_engine"] = arms, ratio
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
