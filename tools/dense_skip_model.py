"""Host-only scheduling model of the masked dense NT launches of a standard block at the headline shape (no GPU call).

    python tools/dense_skip_model.py [draws]

ViT-H/14, batch 64, 257 tokens: the eight dense_nt_kernel launches of a block on 8 XCDs x 32 workgroup slots (one workgroup per
CU).  Workgroups are dispatched in blockIdx order, round-robin over the XCDs, each to the slot of its XCD that frees first
(in-order list scheduling); the launch lasts as long as its fullest XCD.  For Bernoulli(0.5) sample masks the script compares,
against the unmasked launch:
  early exit  - the unmasked order (the all-kept answer of octic_dense_gemm_order_dropped), a dead item returning at once;
  dead first  - the masked kernel's own order (octic_dense_gemm_order_dropped);
  dead last   - the same live deal with the dead full tiles moved behind it;
  adaptive    - octic_dense_gemm_nt_tokens_adaptive's own order and width (octic_dense_gemm_order_adaptive) where it takes the
                launch: 256-wide tiles while live panels * (N / 256) <= CUs, else the 320-wide launch ("-" = not eligible).
With --keep the last part prices the adaptive schedule over the keep probabilities of the headline's 16 standard blocks
(0.74 ... 0.50) instead of Bernoulli(0.5).
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


def order_adaptive(L, N, K, scale):
    """(tm, dead, width) of the adaptive launch, or None where the adaptive kernel does not take it."""
    sc = np.ascontiguousarray(scale, dtype=np.float32)
    cap = 4096
    arrs = [np.zeros(cap, dtype=np.int32) for _ in range(3)]
    width = ctypes.c_int(0)
    g = L.octic_dense_gemm_order_adaptive(B * T, N, K, 0, T, sc.ctypes.data, T, cap, *[a.ctypes.data for a in arrs],
                                          ctypes.addressof(width))
    if g <= 0:
        return None
    return arrs[0][:g].copy(), arrs[2][:g].copy(), width.value


def adaptive_makespan(L, N, K, kept):
    got = order_adaptive(L, N, K, kept.astype(np.float32))
    if got is None:
        return None
    tm, dead, width = got
    return makespan(np.where(tm < 0, 0.0, np.where(dead == 1, DEAD, K // 64 * width / 256.0 + 3.0))), width


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
    args = [a for a in sys.argv[1:] if a != "--keep"]
    draws = int(args[0]) if args else 400
    L = _lib.lib()
    rng = np.random.default_rng(0)
    masks = [(rng.random(B) < 0.5) for _ in range(draws)]
    print(f"{draws} Bernoulli(0.5) masks of {B} samples; launch length relative to the unmasked launch")
    print(f"{'launch':22s} {'tile':>4s} {'grid':>5s} {'live tiles':>10s} {'early exit':>10s} {'dead first':>10s} {'dead last':>10s} {'adaptive':>10s}")
    for name, N, K, mode in LAUNCHES:
        out = (ctypes.c_int * 4)()
        assert L.octic_dense_gemm_plan(B * T, N, K, mode, T, out) == 0
        width = out[0]
        nkt, wf = K // 64, width / 256.0
        tm0, _, part0, front0, _ = order(L, N, K, mode, np.ones(B))
        split = int(part0[front0 == 1].max()) + 1 if front0.any() else 1
        item_cost = lambda front: np.where(front == 1, nkt / split * wf + 3.0, nkt * wf + 3.0)
        base = makespan(np.where(tm0 < 0, 0.0, item_cost(front0)))
        res = {"live": [], "early": [], "first": [], "last": [], "adapt": []}
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
            ad = adaptive_makespan(L, N, K, kept) if mode == 0 else None
            if ad is not None:
                res["adapt"].append(ad[0] / base)
        adapt = f"{np.mean(res['adapt']):10.2f}" if res["adapt"] else f"{'-':>10s}"
        print(f"{name:22s} {width:4d} {len(tm0):5d} {np.mean(res['live']):10.2f} {np.mean(res['early']):10.2f} "
              f"{np.mean(res['first']):10.2f} {np.mean(res['last']):10.2f} {adapt}")
    if "--keep" in sys.argv:
        # the headline's standard blocks: keep probability 0.74 ... 0.50 over 16 blocks, proj's shape (N = K = 1280)
        print("\nadaptive schedule of the N = 1280 launches per standard block (keep probability p), relative to the unmasked launch")
        print(f"{'block':>5s} {'p':>5s} {'live':>6s} {'today':>7s} {'always narrow':>14s} {'adaptive':>9s} {'narrow chosen':>14s}")
        N, K = 1280, 1280
        tm0, _, _, front0, _ = order(L, N, K, 0, np.ones(B))
        base = makespan(np.full(len(tm0), K // 64 * 1.25 + 3.0))
        tot = np.zeros(3)
        for blk, p in enumerate(np.linspace(0.74, 0.50, 16)):
            today, narrow, adapt, chosen, live = [], [], [], 0, []
            for _ in range(draws):
                kept = rng.random(B) < p
                tm, _, _, _, dead = order(L, N, K, 0, kept.astype(np.float32))
                today.append(makespan(np.where(dead == 1, DEAD, K // 64 * 1.25 + 3.0)) / base)
                _lib.route_override(_lib.ROUTE_DENSE_TILE, _lib.DENSE_ADAPT_NARROW)
                narrow.append(adaptive_makespan(L, N, K, kept)[0] / base)
                _lib.route_override(_lib.ROUTE_DENSE_TILE, 0)
                m, w = adaptive_makespan(L, N, K, kept)
                adapt.append(m / base)
                chosen += w == 256
                live.append(kept.mean())
            row = np.array([np.mean(today), np.mean(narrow), np.mean(adapt)])
            tot += row / 16
            print(f"{blk:5d} {p:5.2f} {np.mean(live):6.2f} {row[0]:7.3f} {row[1]:14.3f} {row[2]:9.3f} {chosen / draws:14.2f}")
        print(f"{'mean':>5s} {'':5s} {'':6s} {tot[0]:7.3f} {tot[1]:14.3f} {tot[2]:9.3f}")


if __name__ == "__main__":
    main()
