"""One training step of the attentive-probe grid (octic_vits_amd/classification.py, csrc/attnpool.hip) on one MI355X at the
reference's shape: the 30 AttnPoolClassifier heads of the "patch" source (10 learning rates x 3 weight decays, with the 30
LinearClassifier heads of "cls_avg_patch" the reference always adds) on B 128 images of N 256 float32 patch tokens, D 1280,
C 1000 classes.  Arms, on the same tensors and the same initial weights:

  engine : ClassifierGrid.step_features - the folded formulation on the HIP kernels, fused AdamW
  stock  : the same modules' stock forward (kv projection of every token, SDPA), F.cross_entropy over [B, C, G],
           loss.backward(), torch.optim.AdamW(betas=(0.9, 0.95)) with the reference's groups - float32, eager
  compile: the stock arm's forward under torch.compile (only with --compile, and only where it compiles)

The arms alternate in one process, one step per HIP event pair; min / median / max per arm.  Then, in a pass of its own,
the engine's per-kernel times (KERNEL_TIMER) with each kernel's share of its bound: the larger of FLOPs over the 157.3 TF f32
MFMA peak and algorithmic bytes over the 8 TB/s HBM peak, over the kernel's time.

    python tools/bench_attnpool.py [--iters 7] [--warmup 2] [--compile] [--out profiles/bench_attnpool.txt]
(profiles/bench_attnpool_compile.txt is the run with --compile --iters 5.)
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import copy
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import classification as CL  # noqa: E402
from octic_vits_amd import ops  # noqa: E402

HBM_PEAK = 8.0e12                    # HBM3E spec of the MI355X, as in bench.py
F32_MFMA_PEAK = 157.3e12             # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "n": len(s)}


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


class StockArm:
    def __init__(self, grid, compiled):
        self.mods = copy.deepcopy(grid.classifiers)
        groups = []
        for i, key in enumerate(grid.keys):
            base_lr, wd = grid.hyper[key]
            for name, p in self.mods[i].named_parameters():
                p.grad = None
                groups.append({"params": [p], "base_lr": base_lr, "weight_decay": 0.0 if "bias" in name else wd})
        self.opt = torch.optim.AdamW(groups, lr=0.0, weight_decay=0.0, betas=(0.9, 0.95))
        self.schedule, self.iteration = grid.schedule, grid.iteration

        def forward(feats, labels):
            pred = torch.stack(list(self.mods(feats).values()), dim=-1)
            return F.cross_entropy(pred, labels[:, None].expand(-1, pred.shape[-1]))
        self.forward = torch.compile(forward) if compiled else forward

    def step(self, feats, labels):
        for pg in self.opt.param_groups:
            pg["lr"] = self.schedule[self.iteration] * pg["base_lr"]
        loss = self.forward(feats, labels)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        self.iteration += 1
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--B", type=int, default=128)
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--D", type=int, default=1280)
    ap.add_argument("--C", type=int, default=1000)
    ap.add_argument("--lrs", type=int, default=10)
    ap.add_argument("--wds", type=int, default=3)
    ap.add_argument("--compile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attnpool: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    B, N, D, C = args.B, args.N, args.D, args.C
    grid = CL.ClassifierGrid(None, representations=("patch",), learning_rates=CL.DEFAULT_LEARNING_RATES[:args.lrs],
                             weight_decays=CL.DEFAULT_WEIGHT_DECAYS[:args.wds], batch_size=B, num_classes=C, device=dev,
                             embed_dim=D)
    grid.iteration = grid.warmup_iters                         # the schedule's peak: every step moves the weights
    g = torch.Generator(device=dev).manual_seed(1)
    feats = {"cls_avg_patch": torch.randn(B, 2 * D, generator=g, device=dev), "patch": torch.randn(B, N, D, generator=g, device=dev)}
    labels = torch.randint(0, C, (B,), generator=g, device=dev)
    G = sum(s.G for s in grid.sources if s.attn)
    arms = {"engine": lambda: grid.step_features(feats, labels)}
    stock = StockArm(grid, False)
    arms["stock"] = lambda: stock.step(feats, labels)
    res = {"device": torch.cuda.get_device_name(0), "B": B, "N": N, "D": D, "C": C, "attnpool_classifiers": G,
           "classifiers": len(grid), "what": "ms per training step, one step per event pair, arms alternating, float32"}
    if args.compile:
        try:
            comp = StockArm(grid, True)
            comp.step(feats, labels)
            torch.cuda.synchronize()
            arms["compile"] = lambda: comp.step(feats, labels)
        except Exception as e:                                 # the compiler is optional: say why it is absent
            res["compile"] = f"did not compile: {type(e).__name__}: {str(e)[:200]}"
    else:
        res["compile"] = "not measured (run with --compile)"
    # both arms start from the same weights: the first step's losses agree
    l_engine = float(grid.step_features(feats, labels).mean())
    l_stock = float(stock.step(feats, labels))
    res["first_step_loss"] = {"engine": l_engine, "stock": l_stock}
    for _ in range(args.warmup):
        for fn in arms.values():
            _timed(fn)
    samples = {k: [] for k in arms}
    for _ in range(args.iters):                                # alternating: the arms see the same machine state
        for k, fn in arms.items():
            samples[k].append(_timed(fn))
    res["arms"] = {k: _stats(v) for k, v in samples.items()}
    for k in arms:
        if k != "engine":
            res[f"{k}_over_engine"] = round(res["arms"][k]["median_ms"] / res["arms"]["engine"]["median_ms"], 2)
    # FLOP counts of the two formulations of the AttnPool heads alone (forward + backward, products only)
    res["flops_per_step"] = {"stock_kv_fwd_and_wgrad": 2 * 2.0 * G * B * N * D * 2 * D,
                             "folded_scores_pool_dscores_dfold": 4 * 2.0 * B * N * G * (D // 64) * D,
                             "folded_value_dz_dwv": 3 * 2.0 * B * G * D * D}
    ops.KERNEL_TIMER.enable()
    for _ in range(3):
        grid.step_features(feats, labels)
    kernels = {}
    total = 0.0
    for name, a in sorted(ops.KERNEL_TIMER._agg().items(), key=lambda kv: -kv[1]["total_us"]):
        us = a["avg_us"]
        t_mfma = a["flops_per_launch"] / F32_MFMA_PEAK * 1e6
        t_hbm = a["alg_bytes_per_launch"] / HBM_PEAK * 1e6
        bound = "mfma" if t_mfma >= t_hbm else "hbm"
        kernels[name] = {"launches_per_step": a["launches"] // 3, "avg_us": round(us, 1), "us_per_step": round(a["total_us"] / 3, 1),
                         "bound": bound, "share_of_bound": round(max(t_mfma, t_hbm) / us, 3) if us > 0 else None,
                         "TFLOPs": round(a["flops_per_launch"] / us / 1e6, 1) if us > 0 else None,
                         "GBps": round(a["alg_bytes_per_launch"] / us / 1e3, 1) if us > 0 else None}
        total += a["total_us"] / 3
    ops.KERNEL_TIMER.disable()
    res["engine_kernels"] = kernels
    res["engine_kernel_us_per_step"] = round(total, 1)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
