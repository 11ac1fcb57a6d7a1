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

    python tools/bench_seg_knn.py [--queries 8192] [--keys 262144] [--iters 20] [--out profiles/bench_seg_knn.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402

F32_MFMA_GEMM_TFLOPS = 122.0   # an untuned LDS-tiled f32-MFMA GEMM at 4096^3: the yardstick
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
    knorm = ops.seg_rownorms(K)
    ws = ops.seg_knn_workspace(n, M, D, kmax, ops.KNN_BOTH, 0, dev)
    out4 = [torch.empty(n, kmax, dtype=dt, device=dev) for dt in (torch.int32, torch.float32, torch.int32, torch.float32)]
    votes = torch.empty(2, len(KS), n, L, dtype=torch.uint8, device=dev)

    def engine():
        ops.seg_knn(Q, K, ops.seg_rownorms(Q), knorm, None, kmax, ops.KNN_BOTH, 0, out=out4, workspace=ws)
        ops.seg_knn_vote(out4[0], labels, KS, out=votes[0])
        ops.seg_knn_vote(out4[2], labels, KS, out=votes[1])

    def stock():
        res = {}
        for k in KS:
            for dist in DISTANCES:
                pred = torch.empty(n, L, dtype=torch.uint8, device=dev)
                for i in range(0, n, QUERY_CHUNK):
                    q = Q[i:i + QUERY_CHUNK]
                    if dist == "L2":
                        d = torch.cdist(q, K, p=2)
                    else:
                        d = 1 - (q / torch.norm(q, dim=-1)[:, None]) @ (K / torch.norm(K, dim=-1)[:, None]).T
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
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    # same inputs: how many pixel predictions of the two arms agree (f32 rounding may swap near-tied neighbours)
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
    work = {
        "engine": {"products": 1, "flops": product,
                   "hbm_bytes": 4.0 * D * (M * -(-n // qt) + n * -(-M // kt)) + 2 * 8.0 * n * kmax * (1 + (splits if splits > 1 else 0))
                   + 2.0 * n * L * (kmax + len(KS))},
        # per grid point: queries and keys once per query chunk, the distance matrix written and read by topk, labels gathered
        "stock_torch": {"products": grid, "flops": grid * product,
                        "hbm_bytes": grid * (4.0 * D * (n + M * -(-n // QUERY_CHUNK)) + 2 * 4.0 * n * M) + sum(2.0 * n * L * (k + 1) for k in KS)}}
    out = {"device": torch.cuda.get_device_name(0), "queries": n, "keys": M, "dim": D, "pixels": L, "kmax": kmax, "ks": KS,
           "distances": DISTANCES, "key_splits": splits, "pixel_agreement": agree, "arms": {}}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2] * 1e-3
        out["arms"][name] = dict(_stats(v), products=work[name]["products"], TFLOP=round(work[name]["flops"] / 1e12, 3),
                                 f32_TFLOPs=round(work[name]["flops"] / med / 1e12, 1),
                                 alg_hbm_GB=round(work[name]["hbm_bytes"] / 1e9, 2),
                                 alg_hbm_TBps=round(work[name]["hbm_bytes"] / med / 1e12, 3))
    eng, stk = out["arms"]["engine"]["median_ms"], out["arms"]["stock_torch"]["median_ms"]
    out["engine_vs_stock"] = {"stock_over_engine": round(stk / eng, 3), "engine_not_slower": eng <= stk,
                              "engine_f32_TFLOPs": out["arms"]["engine"]["f32_TFLOPs"],
                              "yardstick_untuned_f32_mfma_gemm_TFLOPs": F32_MFMA_GEMM_TFLOPS}
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


if __name__ == "__main__":
    main()
