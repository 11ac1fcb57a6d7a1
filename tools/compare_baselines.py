"""Octic hybrids against the standard ViTs they replace, on the same engine: the six models of the reference's perf harness
(experiments/complexity.py:19-28) at 224 x 224, batch 64, and the DINOv2 pair (hybrid_dinov2_vit_huge_patch16 vs vit_huge,
one SSLTrainer step on 2 x 224^2 + 8 x 96^2 crops per image, 32 images, as tools/bench_ssl.py).

Per DeiT model: parameters; matmul GFLOP per image (analytic: forward, and forward + backward = 3 x forward); forward-only
images/s with complexity.py's protocol (eval, bf16 autocast, 10 warm-up + 100 timed forwards); the captured train step
(Trainer.capture; drop_path 0.5 for huge, 0.4 for large, experiments/train_deit.py:7-19) in images/s; peak memory; and the
octic / standard ratio of each pair.  Every model runs in a fresh child process under its own `timeout -k 10`; the first
failure stops the run.

    python tools/compare_baselines.py [--batch 64] [--steps 20] [--json out.json] [--skip-dino]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = [("hybrid_deit_huge_patch14", "deit_huge_patch14_LS"), ("d8_inv_early_deit_huge_patch14", "deit_huge_patch14_LS"),
         ("hybrid_deit_large_patch16", "deit_large_patch16_LS"), ("d8_inv_early_deit_large_patch16", "deit_large_patch16_LS")]
DEIT = ["hybrid_deit_huge_patch14", "d8_inv_early_deit_huge_patch14", "deit_huge_patch14_LS",
        "hybrid_deit_large_patch16", "d8_inv_early_deit_large_patch16", "deit_large_patch16_LS"]
DINO = ["hybrid_dinov2_vit_huge_patch16", "vit_huge"]


def matmul_flops(model, img=224, n_classes=None):
    """Forward matmul FLOPs per image.  A standard block: 24 T D^2 (qkv, proj, fc1, fc2) + 4 T^2 D (q k^T, p v).  An octic
    block: the LinearD8 GEMMs are block-diagonal over the irreps - per Linear 24 T cin cout with cin = D_in / 8 against the
    dense 128 T cin cout (x 3 / 16) - and the same attention.  Plus the patch embedding (dense), the invariant projection
    of the d8_inv models and the head."""
    from octic_vits_amd.vit import NestedTensorBlock, Layer_scale_init_Block, Block
    D = model.embed_dim
    p = model.patch_embed.patch_size
    p = p[0] if isinstance(p, tuple) else p
    n = (img // p) ** 2
    T = n + 1 + int(getattr(model, "num_register_tokens", 0) or 0)
    hidden = model.blocks[-1].mlp.fc1.out_features          # (the last block is a standard one in every model here)
    dense_lin = 2 * T * (3 * D * D + D * D + 2 * D * hidden)
    attn = 4 * T * T * D
    f = 0
    for b in model.blocks:
        std = isinstance(b, (NestedTensorBlock, Layer_scale_init_Block, Block))
        f += (dense_lin if std else dense_lin * 3 / 16) + attn
    f += 2 * n * 3 * p * p * D
    if getattr(model, "invariant", False):
        f += 2 * T * model.invariant_proj.in_features * D
    head = getattr(model, "head", None)
    if head is not None and hasattr(head, "in_features"):
        f += 2 * head.in_features * head.out_features
    return float(f)


def child_deit(name, batch, steps):
    import torch
    from octic_vits_amd.deit_models import create_model
    from octic_vits_amd.train import Trainer, synthetic_batch
    dev = torch.device("cuda", 0)
    dp = 0.5 if "huge" in name else 0.4
    torch.manual_seed(0)
    model = create_model(name, num_classes=1000, drop_path_rate=dp, img_size=224).to(dev)
    params = sum(p.numel() for p in model.parameters())
    fwd = matmul_flops(model)
    x, y = synthetic_batch(batch, 1000, dev, 7)
    # forward only: experiments/complexity.py:40-56 (eval, no_grad, bf16 autocast, 10 warm-up + 100 timed)
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(10):
            model(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(100):
            model(x)
        torch.cuda.synchronize()
        t_fwd = (time.perf_counter() - t0) / 100
    torch.cuda.reset_peak_memory_stats()
    tr = Trainer(model)
    gs = tr.capture(x, y, warmup=3)
    for _ in range(3):
        gs.replay(x, y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = gs.replay(x, y)
    torch.cuda.synchronize()
    t_step = (time.perf_counter() - t0) / steps
    return {"model": name, "params": params, "gflop_fwd_per_img": fwd / 1e9, "gflop_step_per_img": 3 * fwd / 1e9,
            "fwd_img_s": batch / t_fwd, "fwd_ms": t_fwd * 1e3, "step_img_s": batch / t_step, "step_ms": t_step * 1e3,
            "step_tflops": 3 * fwd * batch / t_step / 1e12, "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30,
            "loss": float(loss), "batch": batch, "drop_path": dp}


def child_dino(name, batch, steps):
    import torch
    from octic_vits_amd import dinov2_models, ssl as S  # noqa: F401  (dinov2_models registers the hybrid DINOv2 factories)
    from octic_vits_amd.deit_models import create_model
    torch.manual_seed(0)
    if name == "vit_huge":        # configs train/vith16.yaml on ssl_default_config.yaml: layer scale 1e-5, uniform drop path
        make = lambda: create_model(name, img_size=224, drop_path_rate=0.4, drop_path_uniform=True, init_values=1e-5,
                                    block_chunks=0)
    else:
        make = lambda: create_model(name, img_size=224, drop_path_rate=0.4)
    arch = S.SSLMetaArch(make, 1280).cuda()
    params = sum(p.numel() for p in arch.student["backbone"].parameters())
    fwd = 2 * matmul_flops(arch.student["backbone"], 224) + 8 * matmul_flops(arch.student["backbone"], 96)
    tr = S.SSLTrainer(arch, lr=1e-4)
    images = S.synthetic_multicrop_batch(batch, "cuda", seed=5)
    for _ in range(2):
        out = tr.step(images, teacher_temp=0.04, momentum=0.992)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.step(images, teacher_temp=0.04, momentum=0.992)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"model": name, "params": params, "backbone_gflop_fwd_per_img": fwd / 1e9, "ssl_step_ms": dt * 1e3,
            "ssl_img_s": batch / dt, "peak_gib": torch.cuda.max_memory_allocated() / 2 ** 30,
            "ragged_pass": bool(getattr(arch.student["backbone"], "_single_use_pass", False)),
            "losses": {k: float(v) for k, v in out.items()}, "batch": batch}


def run_child(kind, name, batch, steps, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", kind, name,
           "--batch", str(batch), "--steps", str(steps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stderr[-4000:])
        raise SystemExit(f"{name}: child exited with {p.returncode}; stopping at the first failure")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--dino-batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-dino", action="store_true")
    ap.add_argument("--skip-deit", action="store_true")
    ap.add_argument("--models", default=None, help="comma-separated subset of the DeiT models")
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        kind, name = a.child
        res = child_deit(name, a.batch, a.steps) if kind == "deit" else child_dino(name, a.batch, a.steps)
        print(json.dumps(res))
        return
    rows = {}
    for name in ([] if a.skip_deit else a.models.split(",") if a.models else DEIT):
        r = rows[name] = run_child("deit", name, a.batch, a.steps, 420)
        print(f"{name:34s} {r['params'] / 1e6:7.1f} M  {r['gflop_fwd_per_img']:6.1f} GF fwd  {r['gflop_step_per_img']:7.1f} GF step  "
              f"fwd {r['fwd_img_s']:7.1f} img/s  step {r['step_img_s']:7.1f} img/s ({r['step_ms']:.1f} ms, "
              f"{r['step_tflops']:.0f} TFLOP/s)  peak {r['peak_gib']:.1f} GiB", flush=True)
    ratios = {}
    for octic, std in PAIRS:
        if octic in rows and std in rows:
            o, s = rows[octic], rows[std]
            ratios[f"{octic} / {std}"] = {"flop_ratio": s["gflop_fwd_per_img"] / o["gflop_fwd_per_img"],
                                          "fwd_speedup": o["fwd_img_s"] / s["fwd_img_s"],
                                          "step_speedup": o["step_img_s"] / s["step_img_s"],
                                          "param_ratio": s["params"] / o["params"]}
            r = ratios[f"{octic} / {std}"]
            print(f"{octic} vs {std}: FLOP ratio {r['flop_ratio']:.2f}x, forward {r['fwd_speedup']:.2f}x, "
                  f"train step {r['step_speedup']:.2f}x", flush=True)
    dino = {}
    if not a.skip_dino:
        for name in DINO:
            r = dino[name] = run_child("dino", name, a.dino_batch, 5, 540)
            print(f"{name:34s} {r['params'] / 1e6:7.1f} M  ssl step {r['ssl_step_ms']:.1f} ms  {r['ssl_img_s']:.1f} img/s  "
                  f"peak {r['peak_gib']:.1f} GiB  ragged {r['ragged_pass']}", flush=True)
        o, s = dino[DINO[0]], dino[DINO[1]]
        ratios[f"{DINO[0]} / {DINO[1]}"] = {"flop_ratio": s["backbone_gflop_fwd_per_img"] / o["backbone_gflop_fwd_per_img"],
                                            "ssl_step_speedup": o["ssl_img_s"] / s["ssl_img_s"]}
        print(f"{DINO[0]} vs {DINO[1]}: backbone FLOP ratio {ratios[f'{DINO[0]} / {DINO[1]}']['flop_ratio']:.2f}x, "
              f"SSL step {ratios[f'{DINO[0]} / {DINO[1]}']['ssl_step_speedup']:.2f}x", flush=True)
    out = {"deit": rows, "dino": dino, "ratios": ratios}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
