"""Host-only scheduling model of a masked long-K ("ring") LinearD8 launch at the headline shape (no GPU call).

    python tools/ring_skip_model.py [draws]

ViT-H/14, batch 64, T = 257: 257 E m-tiles of two n-chunks (long items) + 4 x 129 one-dimensional m-tiles (short items) on
8 XCDs x 64 workgroup slots.  Workgroups are dispatched in blockIdx order, round-robin over the XCDs, each to the slot of its
XCD that frees first (in-order list scheduling).  For Bernoulli(0.5) sample masks the script compares, against the planned
unmasked launch:
  early exit   - today's planned order (octic_linear_d8_ring_order), a dead item returning at once;
  re-dealt     - the masked kernel's own order (octic_linear_d8_ring_order_dropped: live first, long before short, dealt evenly).
Costs in cycles (tools/ring_trace.py timelines): long 55 k, short 30 k, dead 2.5 k."""
import ctypes
import heapq
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import _lib  # noqa: E402

B, T, SLOTS = 64, 257, 64
M_TILES, N_CHUNKS = [257, 129, 129, 129, 129], [2, 1, 1, 1, 1]
C_LONG, C_SHORT, C_DEAD = 55_000, 30_000, 2_500


def arr(v):
    return (ctypes.c_int * len(v))(*v)


def makespan(order, cost):
    """order: per workgroup (group, item); cost(group, item) -> cycles.  The launch lasts as long as its fullest XCD."""
    end = 0
    for x in range(8):
        slots = [0] * SLOTS
        heapq.heapify(slots)
        for g, i in order[x::8]:
            t = heapq.heappop(slots) + cost(g, i)
            heapq.heappush(slots, t)
            end = max(end, t)
    return end


def dead_tiles(kept, tokens_per_tile, n_tiles):
    tok = np.repeat(kept, T)
    return [not tok[t * tokens_per_tile:(t + 1) * tokens_per_tile].any() for t in range(n_tiles)]


def main():
    draws = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    raw = _lib.lib()
    items = [m * c for m, c in zip(M_TILES, N_CHUNKS)]
    n = sum(items)
    og, oi, od = arr([0] * n), arr([0] * n), arr([0] * n)
    assert raw.octic_linear_d8_ring_order(5, arr(items), arr([20, 10, 10, 10, 10]), SLOTS, og, oi) == 1
    planned = list(zip(og, oi))
    base = makespan(planned, lambda g, i: C_LONG if g == 0 else C_SHORT)
    rng = np.random.default_rng(0)
    early, dealt, live = [], [], []
    for _ in range(draws):
        kept = rng.random(B) < 0.5
        dl, ds = dead_tiles(kept, 64, M_TILES[0]), dead_tiles(kept, 128, M_TILES[1])
        cost = lambda g, i: (C_DEAD if dl[i // 2] else C_LONG) if g == 0 else (C_DEAD if ds[i] else C_SHORT)
        early.append(makespan(planned, cost) / base)
        fl = (ctypes.c_ubyte * len(dl))(*map(int, dl))
        fs = (ctypes.c_ubyte * len(ds))(*map(int, ds))
        assert raw.octic_linear_d8_ring_order_dropped(5, arr(M_TILES), arr([20, 10, 10, 10, 10]), SLOTS, arr(N_CHUNKS), fl, fs, og, oi,
                                                      od) == n
        dealt.append(makespan(list(zip(og, oi)), cost) / base)
        w = 2 * C_LONG * (len(dl) - sum(dl)) + 4 * C_SHORT * (len(ds) - sum(ds))
        live.append(w / (2 * C_LONG * len(dl) + 4 * C_SHORT * len(ds)))
    print(f"planned unmasked launch: {base} cycles; {draws} Bernoulli(0.5) masks of {B} samples")
    print(f"live fraction by item time          {np.mean(live):.2f}")
    print(f"early exit in the planned order     {np.mean(early):.2f}  (min {min(early):.2f}, max {max(early):.2f})")
    print(f"live first, dealt over the XCDs     {np.mean(dealt):.2f}  (min {min(dealt):.2f}, max {max(dealt):.2f})")


if __name__ == "__main__":
    main()
