"""One value-and-gradient evaluation of the segmentation logistic regression on one MI355X: csrc/segeval.hip against the stock
torch composition (F.linear, F.cross_entropy, the two explicit gradient products) on the same resident features.

Shape: N = 3 564 000 patch rows (ADE20K, nine tenths of the training set at 224 x 224), D = 1280, C = 150; the features are
generated on the device from a seed, in chunks.  The two arms alternate in one process, HIP events around each evaluation,
at least 20 evaluations each after warm-up.  TFLOP/s are computed from the shapes (two GEMMs of 2 N C D flops) and set against
the 155 TFLOP/s measured exact-f32 MFMA rate; per-kernel times of the engine arm come from KERNEL_TIMER in a pass of its own
(and from a separate rocprofv3 --kernel-trace --stats run of this program with --engine-only).  One whole fit (--fit-iters
L-BFGS iterations, one C) is timed as a side figure.

    python tools/bench_seg_logreg.py [--rows 3564000] [--iters 20] [--fit-iters 1000] [--out profiles/bench_seg_logreg.json]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402
from octic_vits_amd import segmentation as S  # noqa: E402

F32_MFMA_TFLOPS = 155.0      # measured exact-f32 MFMA rate of the MI355X
HBM_TBPS = 8.0               # HBM3E peak bandwidth


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "n": len(s)}


def features(N, D, C, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = torch.empty(N, D, dtype=torch.float32, device=dev)
    centers = torch.randn(C, D, generator=g, device=dev) * 0.3
    y = torch.randint(0, C, (N,), generator=g, device=dev)
    for i in range(0, N, 262144):                      # standardised-looking rows with class structure, chunk by chunk
        rows = X[i:i + 262144]
        torch.randn(rows.shape, generator=g, device=dev, out=rows)
        rows += centers[y[i:i + 262144]]
    return X, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3_564_000)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--classes", type=int, default=150)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--fit-iters", type=int, default=1000)
    ap.add_argument("--engine-only", action="store_true", help="a few engine evaluations only (the rocprofv3 run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_logreg: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    N, D, C = args.rows, args.dim, args.classes
    X, y64 = features(N, D, C, dev)
    y = y64.to(torch.int32)
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.randn(C, D, generator=g, device=dev) * 0.02
    b = torch.randn(C, generator=g, device=dev) * 0.1
    ldd = ops.seg_ldd(C)
    dl = torch.empty(N, ldd, dtype=torch.float32, device=dev)
    ws = ops.seg_workspace(N, D, C, dev)
    value = torch.empty(1, dtype=torch.float64, device=dev)
    dW, db = torch.empty_like(W), torch.empty_like(b)
    rows = torch.arange(N, device=dev)

    def engine():
        ops.seg_value_dlogits(X, W, b, y, dl, value, ws)
        ops.seg_wgrad(X, dl, W, 1.0, 1.0, dW, db, ws)

    def stock():
        logits = F.linear(X, W, b)
        loss = F.cross_entropy(logits, y64, reduction="sum")
        p = F.softmax(logits, dim=-1)
        p[rows, y64] -= 1
        return loss, p.T @ X + W, p.sum(0)

    if args.engine_only:
        for _ in range(5):
            engine()
        torch.cuda.synchronize()
        print(json.dumps({"engine_only_evaluations": 5}))
        return
    arms = {"engine": engine, "stock_torch": stock}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    # same inputs, same result: the two arms agree before they are timed
    loss, gW, gb = stock()
    agree = {"value_rel": abs(float(value) - float(loss)) / abs(float(loss)),
             "dW_rel": float((dW - gW).abs().max() / gW.abs().max()), "db_rel": float((db - gb).abs().max() / gb.abs().max())}
    del loss, gW, gb
    ms = {k: [] for k in arms}
    for _ in range(max(20, args.iters)):               # alternating: both arms see the same machine state
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    flops = 4.0 * N * C * D
    out = {"device": torch.cuda.get_device_name(0), "rows": N, "dim": D, "classes": C, "dlogits_stride": ldd,
           "slabs": ops.lib().octic_seg_slabs(N, D, C), "features_GB": round(4.0 * N * D / 1e9, 2),
           "alg_TFLOP_per_evaluation": round(flops / 1e12, 3), "agreement": agree,
           "arms": {k: dict(_stats(v), TFLOPs=round(flops / (sorted(v)[len(v) // 2] * 1e-3) / 1e12, 1)) for k, v in ms.items()}}
    eng, stk = out["arms"]["engine"]["median_ms"], out["arms"]["stock_torch"]["median_ms"]
    out["engine_vs_stock"] = {"stock_over_engine": round(stk / eng, 3), "engine_not_slower": eng <= stk,
                              "engine_share_of_f32_mfma_peak": round(flops / (eng * 1e-3) / 1e12 / F32_MFMA_TFLOPS, 3)}
    # per-kernel pass: the time the hardware could not beat is max(flops / MFMA rate, bytes / HBM rate); name the binding one
    ops.KERNEL_TIMER.enable()
    for _ in range(5):
        engine()
    kernels = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    alg = {"seg_forward_kernel": (4.0 * N * (D + ldd), 2.0 * N * C * D),
           "seg_wgrad_kernel": (4.0 * N * D + 4.0 * N * ldd * (D // (256 if D % 256 == 0 and ldd <= 160 else 128 if D % 128 == 0 else 64)),
                                2.0 * N * C * D)}
    for name, (nbytes, fl) in alg.items():
        if name in kernels:
            t_mfma, t_hbm = fl / (F32_MFMA_TFLOPS * 1e12), nbytes / (HBM_TBPS * 1e12)
            kernels[name].update(alg_GB=round(nbytes / 1e9, 2), bound="mfma" if t_mfma >= t_hbm else "hbm",
                                 floor_ms=round(max(t_mfma, t_hbm) * 1e3, 2),
                                 share_of_floor=round(max(t_mfma, t_hbm) * 1e6 / kernels[name]["avg_us"], 3))
    out["engine_kernels"] = kernels
    if args.fit_iters > 0:
        # no pixel labels here: the solver is driven on the class indices directly
        clf = S.LogregClassifier(ignore_labels=(), max_iter=(args.fit_iters,))
        clf.C = 1.0 / N                                 # the data term weighs like the mean cross entropy
        clf.label_dtype, clf.n_pixels_per_sample = torch.int64, 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clf._fit(X, y, torch.arange(C, device=dev))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        info = clf.solver_info_
        out["whole_fit"] = {"seconds": round(dt, 2), "C": clf.C, **info,
                            "ms_per_evaluation_incl_host": round(dt * 1e3 / max(1, info["n_eval"]), 2)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not out["engine_vs_stock"]["engine_not_slower"]:
        raise SystemExit("bench_seg_logreg: the engine's median evaluation is LONGER than the stock composition's")


if __name__ == "__main__":
    main()
