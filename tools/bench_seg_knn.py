"""The k-NN classifier of the segmentation evaluation on one MI355X: ONE fused pass of csrc/segknn.hip (both distances, kmax = 30)
plus the per-pixel vote for 4 neighbour counts, against the stock-torch composition of the reference's KNNClassifier for all 8
grid points (``cdist`` or a normalised matmul, ``topk``, the gather of the neighbours' pixel labels, ``mode``) on the same device.

Shape: n = 8192 queries, M = 262144 keys (one chunk of the reference's train_set_chunk_size), D = 1280, L = 256 pixels per patch;
features and labels are generated on the device from a seed.  The two arms alternate in one process, HIP events around each
whole grid, 5 warm-up and 20 timed runs.  Each arm is reported with ITS OWN work: the engine does one n x M x D product, the
composition 8; TFLOP/s are those flops over the median time, HBM bytes are the algorithmic bytes computed from the shapes (the
engine: keys once per query tile, queries once per key tile, lists, neighbour labels; the composition additionally writes and
re-reads every distance matrix).  The engine's TFLOP/s stand next to the 122 TFLOP/s of an untuned f32-MFMA GEMM as a yardstick,
not a threshold.  The one condition: the engine's full grid must not take longer than the composition's.

``--dtype bfloat16`` is the reference's shipped configuration (``classifiers_kwargs: {knn: {dtype: bfloat16}}``): the engine arm
casts the query batch to bf16 inside the timed region (as ``KNNClassifier.predict_grid`` does; the keys are cast once, as in
``fit``) and runs the bf16-MFMA pass, the composition runs the reference's own arithmetic on bf16 tensors, and a third arm,
``engine_float32``, runs the float32 pass on the same data in the same alternation - so the bf16 time, the f32 time and the
composition's time come from ONE run.  Two conditions then: the bf16 grid must take no longer than the f32 grid, and no longer
than the bf16 composition.  The engine's TFLOP/s stand next to the bf16 MFMA peak (2.5 PFLOP/s dense).

    python tools/bench_seg_knn.py [--dtype float32|bfloat16] [--queries 8192] [--keys 262144] [--iters 20] [--out FILE]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402

F32_MFMA_GEMM_TFLOPS = 122.0   # an untuned LDS-tiled f32-MFMA GEMM at 4096^3: the yardstick
BF16_MFMA_PEAK_TFLOPS = 2500.0  # the dense bf16 MFMA peak of one MI355X
KS = (1, 3, 10, 30)
DISTANCES = ("cosine", "L2")
QUERY_CHUNK = 1024             # the reference's inference_bs


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--keys", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--pixels", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", choices=("float32", "bfloat16"), default="float32")
    ap.add_argument("--engine-only", action="store_true", help="a few engine passes only (a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_knn: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    n, M, D, L = args.queries, args.keys, args.dim, args.pixels
    g = torch.Generator(device=dev).manual_seed(0)
    centers = torch.randn(150, D, generator=g, device=dev) * 0.3
    kcls = torch.randint(0, 150, (M,), generator=g, device=dev)
    K = torch.randn(M, D, generator=g, device=dev) + centers[kcls]
    Q = torch.randn(n, D, generator=g, device=dev) + centers[torch.randint(0, 150, (n,), generator=g, device=dev)]
    labels = (kcls[:, None] + 1).to(torch.uint8).repeat(1, L)
    labels[torch.rand(M, L, generator=g, device=dev) < 0.1] = 0
    kmax = KS[-1]
    dtype = getattr(torch, args.dtype)
    bf16 = dtype == torch.bfloat16
    Kd = K.to(dtype)                                   # the resident keys of the arm's dtype: cast once, as in fit
    knorm = {torch.float32: ops.seg_rownorms(K)}
    knorm[dtype] = ops.seg_rownorms(Kd)
    ws = ops.seg_knn_workspace(n, M, D, kmax, ops.KNN_BOTH, 0, dev)
    out4 = [torch.empty(n, kmax, dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32, torch.float32)]
    votes = torch.empty(2, len(KS), n, L, dtype=torch.uint8, device=dev)

    def engine_of(keys):
        def run():
            q = Q.to(keys.dtype)                       # a copy only at bf16: the cast of the query batch
            ops.seg_knn(q, keys, ops.seg_rownorms(q), knorm[keys.dtype], None, kmax, ops.KNN_BOTH, 0, out=out4, workspace=ws)
            ops.seg_knn_vote(out4[0], labels, KS, out=votes[0])
            ops.seg_knn_vote(out4[2], labels, KS, out=votes[1])
        return run

    engine = engine_of(Kd)

    def stock():
        res = {}
        for k in KS:
            for dist in DISTANCES:
                pred = torch.empty(n, L, dtype=torch.uint8, device=dev)
                for i in range(0, n, QUERY_CHUNK):
                    q = Q[i:i + QUERY_CHUNK].to(dtype)
                    if dist == "L2":
                        d = torch.cdist(q, Kd, p=2)
                    else:
                        d = 1 - (q / torch.norm(q, dim=-1)[:, None]) @ (Kd / torch.norm(Kd, dim=-1)[:, None]).T
                    idx = torch.topk(d, k, dim=-1, largest=False).indices
                    pred[i:i + QUERY_CHUNK] = labels[idx].mode(dim=1).values
                res[(k, dist)] = pred
        return res

    if args.engine_only:
        for _ in range(5):
            engine()
        torch.cuda.synchronize()
        print(json.dumps({"engine_only_passes": 5}))
        return
    arms = {"engine": engine, "stock_torch": stock}
    if bf16:
        arms["engine_float32"] = engine_of(K)
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    # same inputs: how many pixel predictions of the two arms agree (f32 rounding may swap near-tied neighbours; at bf16 the
    # composition ranks 8-bit distances, which tie in bulk, so its neighbour sets are one arbitrary choice among many)
    engine()
    res = stock()
    agree = {f"{k}_{d}": round(float((votes[1 - DISTANCES.index(d), KS.index(k)] == res[(k, d)]).float().mean()), 6)
             for k in KS for d in DISTANCES}
    del res
    ms = {k: [] for k in arms}
    for _ in range(max(20, args.iters)):               # alternating: both arms see the same machine state
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    product = 2.0 * n * M * D
    splits, qt, kt, _ = ops.seg_knn_plan(n, M, D, kmax, ops.KNN_BOTH)
    grid = len(KS) * len(DISTANCES)
    es = float(Kd.element_size())

    def engine_bytes(esize):
        return (esize * D * (M * -(-n // qt) + n * -(-M // kt)) + 2 * 8.0 * n * kmax * (1 + (splits if splits > 1 else 0))
                + 2.0 * n * L * (kmax + len(KS)))

    work = {
        "engine": {"products": 1, "flops": product, "hbm_bytes": engine_bytes(es)},
        "engine_float32": {"products": 1, "flops": product, "hbm_bytes": engine_bytes(4.0)},
        # per grid point: queries and keys once per query chunk, the distance matrix written and read by topk, labels gathered
        "stock_torch": {"products": grid, "flops": grid * product,
                        "hbm_bytes": grid * (es * D * (n + M * -(-n // QUERY_CHUNK)) + 2 * es * n * M) + sum(2.0 * n * L * (k + 1) for k in KS)}}
    out = {"device": torch.cuda.get_device_name(0), "dtype": args.dtype, "queries": n, "keys": M, "dim": D, "pixels": L, "kmax": kmax, "ks": KS,
           "distances": DISTANCES, "key_splits": splits, "pixel_agreement": agree, "arms": {}}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2] * 1e-3
        out["arms"][name] = dict(_stats(v), products=work[name]["products"], TFLOP=round(work[name]["flops"] / 1e12, 3),
                                 TFLOPs=round(work[name]["flops"] / med / 1e12, 1),
                                 alg_hbm_GB=round(work[name]["hbm_bytes"] / 1e9, 2),
                                 alg_hbm_TBps=round(work[name]["hbm_bytes"] / med / 1e12, 3))
    eng, stk = out["arms"]["engine"]["median_ms"], out["arms"]["stock_torch"]["median_ms"]
    out["engine_vs_stock"] = {"stock_over_engine": round(stk / eng, 3), "engine_not_slower": eng <= stk,
                              "engine_TFLOPs": out["arms"]["engine"]["TFLOPs"]}
    if bf16:
        f32 = out["arms"]["engine_float32"]["median_ms"]
        out["engine_vs_stock"].update(bf16_mfma_peak_TFLOPs=BF16_MFMA_PEAK_TFLOPS,
                                      fraction_of_bf16_mfma_peak=round(out["arms"]["engine"]["TFLOPs"] / BF16_MFMA_PEAK_TFLOPS, 4))
        out["bfloat16_vs_float32"] = {"float32_over_bfloat16": round(f32 / eng, 3), "bfloat16_not_slower": eng <= f32}
    else:
        out["engine_vs_stock"]["yardstick_untuned_f32_mfma_gemm_TFLOPs"] = F32_MFMA_GEMM_TFLOPS
    ops.KERNEL_TIMER.enable()
    for _ in range(5):
        engine()
    out["engine_kernels"] = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not out["engine_vs_stock"]["engine_not_slower"]:
        raise SystemExit("bench_seg_knn: the engine's full grid takes LONGER than the stock composition's")
    if bf16 and not out["bfloat16_vs_float32"]["bfloat16_not_slower"]:
        raise SystemExit("bench_seg_knn: the bfloat16 grid takes LONGER than the float32 grid")


if __name__ == "__main__":
    main()
