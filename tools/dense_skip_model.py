"""Host-only scheduling model of the masked dense NT launches of a standard block at the headline shape (no GPU call).

    python tools/dense_skip_model.py [draws]

ViT-H/14, batch 64, 257 tokens: the eight dense_nt_kernel launches of a block on 8 XCDs x 32 workgroup slots (one workgroup per
CU).  Workgroups are dispatched in blockIdx order, round-robin over the XCDs, each to the slot of its XCD that frees first
(in-order list scheduling); the launch lasts as long as its fullest XCD.  For Bernoulli(0.5) sample masks the script compares,
against the unmasked launch:
  early exit  - the unmasked order (the all-kept answer of octic_dense_gemm_order_dropped), a dead item returning at once;
  dead first  - the masked kernel's own order (octic_dense_gemm_order_dropped);
  dead last   - the same live deal with the dead full tiles moved behind it.
Costs in units of one K-tile of the 256-wide tile (dense_plan_nt's model): a full tile nkt * width / 256 + 3, a split part
nkt / split * width / 256 + 3 (the reducer's 17 units are left out: they are the same in every column), a dead tile DEAD."""
import ctypes
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import _lib  # noqa: E402

B, T, SLOTS = 64, 257, 32
DEAD = 1.0
LAUNCHES = [("qkv forward", 3840, 1280, 0), ("proj", 1280, 1280, 0), ("fc1 + factor", 5120, 1280, 4), ("fc2", 1280, 5120, 0),
            ("fc2 input gradient", 5120, 1280, 5), ("fc1 input gradient", 1280, 5120, 0), ("proj input gradient", 1280, 1280, 0),
            ("qkv input gradient", 1280, 3840, 0)]


def order(L, N, K, mode, scale):
    sc = np.ascontiguousarray(scale, dtype=np.float32)
    cap = 4096
    arrs = [np.zeros(cap, dtype=np.int32) for _ in range(5)]
    g = L.octic_dense_gemm_order_dropped(B * T, N, K, mode, T, sc.ctypes.data, T, cap, *[a.ctypes.data for a in arrs])
    assert g > 0
    return [a[:g].copy() for a in arrs]       # tm, tn, part, front, dead


def makespan(costs):
    end = 0.0
    for x in range(8):
        slots = [0.0] * SLOTS
        heapq.heapify(slots)
        for c in costs[x::8]:
            t = heapq.heappop(slots) + c
            heapq.heappush(slots, t)
            end = max(end, t)
    return end


def main():
    draws = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    L = _lib.lib()
    rng = np.random.default_rng(0)
    masks = [(rng.random(B) < 0.5) for _ in range(draws)]
    print(f"{draws} Bernoulli(0.5) masks of {B} samples; launch length relative to the unmasked launch")
    print(f"{'launch':22s} {'tile':>4s} {'grid':>5s} {'live tiles':>10s} {'early exit':>10s} {'dead first':>10s} {'dead last':>10s}")
    for name, N, K, mode in LAUNCHES:
        out = (ctypes.c_int * 4)()
        assert L.octic_dense_gemm_plan(B * T, N, K, mode, T, out) == 0
        width = out[0]
        nkt, wf = K // 64, width / 256.0
        tm0, _, part0, front0, _ = order(L, N, K, mode, np.ones(B))
        split = int(part0[front0 == 1].max()) + 1 if front0.any() else 1
        item_cost = lambda front: np.where(front == 1, nkt / split * wf + 3.0, nkt * wf + 3.0)
        base = makespan(np.where(tm0 < 0, 0.0, item_cost(front0)))
        res = {"live": [], "early": [], "first": [], "last": []}
        for kept in masks:
            tm, _, _, front, dead = order(L, N, K, mode, kept.astype(np.float32))
            cost = np.where(tm < 0, 0.0, np.where(dead == 1, DEAD, item_cost(front)))
            res["first"].append(makespan(cost) / base)
            tail = int((front == 1).sum() + (tm < 0).sum())
            full = cost[tail:]
            d = dead[tail:] == 1
            res["last"].append(makespan(np.concatenate([cost[:tail], full[~d], full[d]])) / base)
            # the unmasked order with the same panels dead
            dead_panel = {int(t) for t, dd in zip(tm, dead) if dd}
            c0 = np.where(tm0 < 0, 0.0, np.where(np.isin(tm0, list(dead_panel)), DEAD, item_cost(front0)))
            res["early"].append(makespan(c0) / base)
            res["live"].append(1.0 - dead.sum() / float((tm >= 0).sum()))
        print(f"{name:22s} {width:4d} {len(tm0):5d} {np.mean(res['live']):10.2f} {np.mean(res['early']):10.2f} "
              f"{np.mean(res['first']):10.2f} {np.mean(res['last']):10.2f}")


if __name__ == "__main__":
    main()
