"""The k-NN classification evaluation on one MI355X: the fused neighbour search of csrc/knn_cls.hip (kmax = 200) plus the
softmax vote for the reference's nb_knn = (10, 20, 100, 200) with device hit counters, against the stock-torch composition of the
reference's KnnModule (``torch.mm`` -> ``topk(200)`` -> ``gather`` -> ``softmax`` -> ``one_hot`` product -> prefix sums, then the
top-1 / top-5 hits of every k from ``topk(5)``) on the same device, in batches of 256 queries as the reference runs it.

Shape: n = 8192 queries, M = 262144 keys, D = 1280, C = 1000 classes; L2-normalised clustered features and labels are generated on
the device from a seed.  The protocol is tools/bench_seg_knn.py's: the two arms alternate in one process, HIP events around each
whole evaluation, 5 warm-up and 20 timed runs; TFLOP/s are the 2 n M D flops of the one similarity product over the median time.
No target ratio is set: both times are recorded whichever is larger.  "Outside the MFMA loop" is measured, not modelled: the
same search at kmax = 1 keeps the product and the one-compare filter but almost no list work, so
(engine - search at kmax = 1) / engine is the share of the inserts, the merge of the key-axis splits and the vote.

    python tools/bench_knn_cls.py [--queries 8192] [--keys 262144] [--iters 20] [--out profiles/bench_knn_cls.txt]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402

NB_KNN = (10, 20, 100, 200)
T = 0.07
STOCK_BATCH = 256              # the reference's batch_size
IMAGENET = (50_000, 1_281_167, 1280)


def _stats(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--keys", type=int, default=262144)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_knn_cls: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    n, M, D, C = args.queries, args.keys, args.dim, args.classes
    kmax = NB_KNN[-1]
    g = torch.Generator(device=dev).manual_seed(0)
    centers = torch.randn(C, D, generator=g, device=dev) * 0.3
    labels = torch.randint(0, C, (M,), generator=g, device=dev)
    targets = torch.randint(0, C, (n,), generator=g, device=dev)
    K = torch.nn.functional.normalize(torch.randn(M, D, generator=g, device=dev) + centers[labels], dim=1)
    Q = torch.nn.functional.normalize(torch.randn(n, D, generator=g, device=dev) + centers[targets], dim=1)
    ws = ops.knn_topk_workspace(n, M, D, kmax, 0, dev)
    lists = (torch.empty(n, kmax, dtype=torch.int32, device=dev), torch.empty(n, kmax, dtype=torch.float32, device=dev))
    one = (torch.empty(n, 1, dtype=torch.int32, device=dev), torch.empty(n, 1, dtype=torch.float32, device=dev))
    ws1 = ops.knn_topk_workspace(n, M, D, 1, 0, dev)
    probas = torch.empty(len(NB_KNN), n, C, dtype=torch.float32, device=dev)
    counters = torch.zeros(len(NB_KNN), 2, dtype=torch.int64, device=dev)
    stock_hits = torch.zeros(len(NB_KNN), 2, dtype=torch.int64, device=dev)
    KT = K.T                                        # the reference keeps the transposed view (train_features_rank_T)

    def engine():
        counters.zero_()
        ops.knn_topk(Q, K, kmax, 0, out=lists, workspace=ws)
        ops.knn_vote(lists[1], lists[0], labels, C, 1 / T, NB_KNN, out=probas, targets=targets, counters=counters)

    def search_k1():
        ops.knn_topk(Q, K, 1, 0, out=one, workspace=ws1)

    def stock():
        stock_hits.zero_()
        for i in range(0, n, STOCK_BATCH):
            q, t = Q[i:i + STOCK_BATCH], targets[i:i + STOCK_BATCH]
            sims, idx = torch.mm(q, KT).topk(kmax, largest=True, sorted=True)
            nl = torch.gather(labels.view(1, -1).expand(len(q), -1), 1, idx)
            w = torch.softmax(sims / T, 1)
            votes = torch.nn.functional.one_hot(nl, num_classes=C) * w.view(len(q), -1, 1)
            for j, k in enumerate(NB_KNN):
                top5 = votes[:, :k, :].sum(1).topk(5, dim=1).indices
                stock_hits[j, 0] += (top5[:, 0] == t).sum()
                stock_hits[j, 1] += (top5 == t[:, None]).any(1).sum()

    arms = {"engine": engine, "stock_torch": stock, "search_kmax1": search_k1}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    agree = {"engine_hits": counters.tolist(), "stock_hits": stock_hits.tolist()}
    ms = {k: [] for k in arms}
    for _ in range(max(20, args.iters)):               # alternating: the arms see the same machine state
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    product = 2.0 * n * M * D
    splits, qt, kt, _ = ops.knn_topk_plan(n, M, D, kmax)
    out = {"device": torch.cuda.get_device_name(0), "queries": n, "keys": M, "dim": D, "classes": C, "kmax": kmax, "nb_knn": NB_KNN,
           "temperature": T, "stock_batch": STOCK_BATCH, "key_splits": splits, "tile": [qt, kt], "hits_top1_top5_per_k": agree,
           "arms": {}}
    for name, v in ms.items():
        med = sorted(v)[len(v) // 2] * 1e-3
        out["arms"][name] = dict(_stats(v), TFLOP=round(product / 1e12, 3), f32_TFLOPs=round(product / med / 1e12, 1))
    eng, stk, k1 = (out["arms"][a]["median_ms"] for a in ("engine", "stock_torch", "search_kmax1"))
    rate = product / (eng * 1e-3)
    full = 2.0 * IMAGENET[0] * IMAGENET[1] * IMAGENET[2]
    out["engine_vs_stock"] = {"stock_over_engine": round(stk / eng, 3), "engine_faster": eng < stk,
                              "share_outside_the_mfma_loop": round(max(0.0, eng - k1) / eng, 3)}
    out["imagenet_extrapolation"] = {"note": "EXTRAPOLATED from the measured engine rate, not measured",
                                     "queries_keys_dim": IMAGENET, "TFLOP": round(full / 1e12, 1), "seconds": round(full / rate, 2)}
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


if __name__ == "__main__":
    main()
