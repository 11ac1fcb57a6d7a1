"""Warm back-to-back launches of the eight dense_nt_kernel shapes of a standard block (ViT-H/14, batch 64, 257 tokens) under a
stochastic-depth mask.

    python tools/bench_dense_skip.py [--iters 30] [--json FILE]

Four cases per shape: unmasked (sample_scale None), all kept (prices the bitmap prologue: same tiles, same order), a fixed
Bernoulli(0.5) mask (seed 0), all dropped (prices the dead tile).  Each case is timed as `iters` launches between two events
after a warm-up, microseconds per launch.  The shapes run with functional.DENSE_NARROW_DROPPED off (the masked launch at the
plan's width); the launches octic_dense_gemm_nt_tokens_adaptive takes get a second row with it on ("... adaptive") and those
octic_dense_gemm_nt_tokens_adaptive_cls takes a third with the class-token rows inside the main launch ("... folded").  Below
the table: folded against adaptive + class-token launches at 32 / 38 / 45 / 52 / 64 of 64 kept for K = 1280 / 3840 / 5120 - what
functional.DENSE_CLS_FOLD_MIN_DROP rests on."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import functional, ops  # noqa: E402

B, T = 64, 257
SHAPES = [("qkv forward", 3840, 1280, 0), ("proj", 1280, 1280, 0), ("fc1 + factor", 5120, 1280, 4), ("fc2", 1280, 5120, 0),
          ("fc2 input gradient", 5120, 1280, 5), ("fc1 input gradient", 1280, 5120, 0), ("proj input gradient", 1280, 1280, 0),
          ("qkv input gradient", 1280, 3840, 0)]


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    bern = (torch.rand(B, generator=g, device=dev) < 0.5).float() * 2.0
    masks = {"unmasked": None, "all kept": torch.full((B,), 2.0, device=dev), "bernoulli": bern,
             "all dropped": torch.zeros(B, device=dev)}
    rows = []
    print(f"kept samples of the Bernoulli mask: {int((bern != 0).sum())} of {B}")
    print(f"{'launch':30s} " + " ".join(f"{k:>12s}" for k in masks))
    for name, N, K, mode in SHAPES:
        a = torch.randn(B * T, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(N, K, device=dev) * K ** -0.5).to(torch.bfloat16)
        h = torch.rand(B * T, N, device=dev).to(torch.bfloat16) if mode == 5 else None
        for adaptive, fold in ((False, False), (True, False), (True, True)):
            if adaptive and not ops.dense_plan_adaptive(B * T, N, K, mode, T, T)[0]:
                continue
            if fold and not ops.dense_plan_adaptive_cls(B * T, N, K, mode, T, T)[0]:
                continue
            functional.DENSE_NARROW_DROPPED = adaptive
            functional.DENSE_CLS_FOLD = fold
            res = {}
            for label, ss in masks.items():
                fn = lambda: ops.dense_gemm_nt(a, w, mode, h=h, want_colsum=mode == 5, tokens=T, sample_scale=ss,
                                               rows_per_sample=T if ss is not None else 0, fold_cls=fold)
                res[label] = timed(fn, args.iters)
            label = name + (" folded" if fold else " adaptive" if adaptive else "")
            rows.append(dict(launch=label, N=N, K=K, mode=mode, us=res))
            print(f"{label:30s} " + " ".join(f"{res[k]:12.1f}" for k in masks))
    # the class-token rows inside the main launch against the launches behind it, by kept count (kept samples spread over the batch)
    functional.DENSE_NARROW_DROPPED = functional.DENSE_CLS_FOLD = True
    kepts = (32, 38, 45, 52, 64)
    fold_rows = []
    print(f"{'N 1280, kept of 64:':30s} " + " ".join(f"{k:>12d}" for k in kepts))
    for K in (1280, 3840, 5120):
        a = torch.randn(B * T, K, device=dev).to(torch.bfloat16)
        w = (torch.randn(1280, K, device=dev) * K ** -0.5).to(torch.bfloat16)
        for fold in (False, True):
            res = {}
            for kept in kepts:
                keep = [1.0] * kept + [0.0] * (B - kept)
                ss = torch.tensor([2.0 * keep[(b * 37) % B] for b in range(B)], device=dev)
                fn = lambda: ops.dense_gemm_nt(a, w, 0, tokens=T, sample_scale=ss, rows_per_sample=T, fold_cls=fold)
                res[kept] = timed(fn, args.iters)
            label = f"K {K} " + ("folded" if fold else "adaptive + class-token")
            fold_rows.append(dict(launch=label, N=1280, K=K, us=res))
            print(f"{label:30s} " + " ".join(f"{res[k]:12.1f}" for k in kepts))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(batch=B, tokens=T, kept=int((bern != 0).sum()), iters=args.iters, rows=rows, fold_rows=fold_rows),
                      f, indent=1)


if __name__ == "__main__":
    main()
