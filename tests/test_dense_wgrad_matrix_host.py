"""CPU-only side of tests/test_dense_wgrad_matrix_gpu.py: its shape tables against the library's plan queries (the library counts
256 compute units without a device, the MI355X's own number) and against a few lines that restate the kernel's slab, tile-list
and liveness rules; the exactness assertions of its operand generator; and what the TN launchers refuse before any launch -
among it the two limits the matrix found missing: a forced slab count above the 16 the workspace query sizes for, and a row
stride shorter than the row on the wide path."""
import pytest
import torch

import test_dense_wgrad_matrix_gpu as T
from octic_vits_amd import _lib

ESHAPE, EALIGN = -1, -2
PLAN = "octic_dense_wgrad_plan"


def _knob(value):
    return T.slabs_knob(value)


def test_the_tables_reach_every_branch():
    widths, slab_counts, nkt_seen = set(), set(), set()
    # 1. steps per slab under S = 1: the prologue issues min(6, 4 nkt) units, the loop is steady for t < nkt - 2
    assert tuple(T.steps_of(M) for M in T.STEPS_M) == T.STEPS_NKT and set(T.STEPS_NKT) == set(range(1, 7))
    for N, K in T.WIDE_NK:
        w = T.width_of(N, K)
        widths.add(w)
        with _knob(1):
            for M in T.STEPS_M:
                assert _lib.plan(PLAN, M, N, 0, K, max(N, K)) == (w, 1, 1, 0), (M, N, K)
                nkt_seen.add((w, T.steps_of(M)))
    assert nkt_seen == {(w, n) for w in (256, 320) for n in range(1, 7)}
    assert {M % T.STEP for M in T.STEPS_M} >= {0, 1, 63}             # full, one-row and 63-row last steps
    # 2. row slabs: the plan's S and the steps of every slab
    for M, forced, S, per_slab in T.SLABS:
        assert tuple(s1 - s0 for s0, s1 in T.slab_steps(M, S)) == per_slab and sum(per_slab) == T.steps_of(M), (M, S)
        assert min(per_slab) >= 2 or S == 1
        for N, K in T.WIDE_NK:
            with _knob(forced):
                assert _lib.plan(PLAN, M, N, 0, K, max(N, K)) == (T.width_of(N, K), 1, S, 0), (M, forced, N, K)
                need = _lib.lib().octic_dense_wgrad_workspace_bytes(M, N, K)
            assert need >= S * 256 * T.width_of(N, K) * 4 + 4096
        if forced:
            assert T.forced_slabs(M, forced) == S
        slab_counts.add(S)
    assert slab_counts == {1, 2, 3, 5, 9, 16}
    assert (130, 2, 1, (3,)) in T.SLABS and (2049, 0, 16) in [row[:3] for row in T.SLABS]
    # 3. tile-list decode: every r8 with q8 = 0, 1, 2; the decode is a bijection onto the tile list at each count
    seen = set()
    for width, table in ((256, T.DECODE_256), (320, T.DECODE_320)):
        for a, b in table:
            N, K = 256 * a, width * b
            assert (T.width_of(N, K), T.tiles_of(N, K)) == (width, a * b)
            tiles = a * b
            got = [T.decode(tiles, j) for j in range((tiles + 7) // 8 * 8)]
            assert sorted(t for t in got if t is not None) == list(range(tiles))
            for M, forced in T.DECODE_MS:
                with _knob(forced):
                    assert _lib.plan(PLAN, M, N, 0, K, max(N, K)) == (width, tiles, T.forced_slabs(M, forced), 0), (M, N, K, forced)
            seen.add((width, tiles & 7, tiles >> 3))
    assert sorted(a * b for a, b in T.DECODE_256) == list(range(1, 18))
    assert {(r8, q8) for w, r8, q8 in seen if w == 256} == {(t & 7, t >> 3) for t in range(1, 18)}
    assert {r8 for w, r8, _ in seen if w == 256} == set(range(8)) and {q8 for w, _, q8 in seen if w == 256} == {0, 1, 2}
    assert {a * b for a, b in T.DECODE_320} == {1, 3, 5, 7, 9}
    assert [T.forced_slabs(M, f) for M, f in T.DECODE_MS] == [1, 2, 3]
    assert max(a for a, _ in T.DECODE_256) * 256 == 4352               # the largest output: 4352 x 256
    # 4. pair: the seam of the joint tile list at tiles0 = 1 .. 6, both widths, four strides
    seams = set()
    for N0, N1, K in T.PAIR_CASES:
        width = T.width_of(N0 + N1, K)
        widths.add(width)
        seams.add((N0 // 256) * (K // width))
        lds = [ld for ld, _ in T.pair_strides(N0, N1, K)]
        assert len(set(lds)) == 4 and all(ld % 8 == 0 for ld in lds)
        assert all(ld >= n + off for (ld, off), n in zip(T.pair_strides(N0, N1, K), (N0, K, N1, K)))
        for M, forced in T.PAIR_MS:
            with _knob(forced):
                want = (width, ((N0 + N1) // 256) * (K // width), T.forced_slabs(M, forced), 0)
                assert _lib.plan(PLAN, M, N0, N1, K, max(lds)) == want, (M, N0, N1, K)
    assert seams == {1, 2, 3, 4, 5, 6}
    assert {(N0 // 256) * (K // T.width_of(N0, K)) for N0 in T.PAIR_N for K in T.PAIR_K} == {1, 2, 3, 4, 6}   # why PAIR_EXTRA
    assert [T.forced_slabs(M, f) for M, f in T.PAIR_MS] == [1, 2]
    # 6. masked: live steps per slab 0 .. 3 at both widths (the width does not enter the rule: every row runs at both)
    live = set()
    for rps, counts, slabs in T.MASKED.values():
        for B in counts:
            M = B * rps
            masks = T.masks_of(B)
            assert len(masks) == (2 ** B if B <= T.EVERY_MASK_UP_TO else 10)
            for forced in slabs:
                S = T.forced_slabs(M, forced)
                for N, K in T.WIDE_NK:
                    with _knob(forced):
                        assert _lib.plan(PLAN, M, N, 0, K, max(N, K)) == (T.width_of(N, K), 1, S, 0)
                for mask in masks.values():
                    for (s0, s1), n in zip(T.slab_steps(M, S), T.live_steps(M, rps, mask, S)):
                        live.add((s1 - s0, n))
    assert {n for _, n in live} >= {0, 1, 2, 3}
    # ... and each of them in a short slab: 0 and 1 live steps under the 4-unit prologue's nkt = 1 and the drain-only nkt = 2
    assert live >= {(1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3)}
    assert {rps for rps, _, _ in T.MASKED.values()} == {64, 65, 1, 37}
    assert [(rps * B) for rps, counts, _ in T.MASKED.values() for B in counts] == [64, 128, 192, 256, 320, 325, 129, 259]
    rps, B, N0, N1, K, forced = T.PAIR_MASKED
    with _knob(forced):
        assert _lib.plan(PLAN, rps * B, N0, N1, K, max(ld for ld, _ in T.pair_strides(N0, N1, K))) == (256, (N0 + N1) // 256, 2, 0)
    # 7. narrow: S = 1, 2, 8 and the cap 32; slab boundaries inside a 32-row stage
    narrow_S = set()
    for N, K in T.NARROW_NK:
        assert T.width_of(N, K) == 64
        widths.add(64)
        tiles = T.tiles_of(N, K)
        assert tiles <= 16
        for M in T.NARROW_M:
            S = T.narrow_slabs(M, tiles)
            assert _lib.plan(PLAN, M, N, 0, K, max(N, K) + 8) == (64, tiles, S, 0), (M, N, K)
            assert _lib.lib().octic_dense_wgrad_workspace_bytes(M, N, K) == tiles * S * 64 * 64 * 4 + 4096
            narrow_S.add((M, S))
    assert narrow_S == {(1, 1), (31, 1), (32, 1), (33, 1), (127, 1), (129, 1), (257, 2), (1027, 8), (4099, 32)}
    assert -(-129 // T.STAGE) == 5 and -(-257 // T.STAGE) == 9 and -(-4099 // T.STAGE) == 129
    for M, S in ((257, 2), (1027, 8), (4099, 32)):
        cuts = [M * s // S for s in range(1, S)]
        assert any((M * (s + 1) // S - M * s // S) % T.STAGE for s in range(S))      # a last stage with rows past r1
        assert S == 2 or any(c % T.STAGE for c in cuts)                                # a slab that begins inside a stage
    for M, N, K in T.NARROW_STRIDED:
        assert _lib.plan(PLAN, M, N, 0, K, max(N, K) + 8) == (64, T.tiles_of(N, K), T.narrow_slabs(M, T.tiles_of(N, K)), 0)
    M, N, K, rps = T.NARROW_MASK
    assert T.width_of(N, K) == 64 and M % rps == 0
    assert widths == {64, 256, 320}
    # selector and random cases: one per kernel
    assert [T.width_of(N, K) for _, N, K in T.SELECTOR] == [256, 320, 64] == [T.width_of(N, K) for _, N, K in T.RANDOM]
    assert all(M <= min(N, K) for M, N, K in T.SELECTOR)
    assert _lib.route_override(_lib.ROUTE_WGRAD_SLABS, 0) == 0


def test_operands_are_exact_at_the_largest_shape():
    """The generator's own assertions at the largest M of the tables, the selector problems, and the limit they guard."""
    largest = max(max(T.NARROW_M), max(T.STEPS_M), max(row[0] for row in T.SLABS))
    assert largest == 4099
    dy, x, want = T.dyadic(largest, 320, 192)                       # asserts 96 M < 2^24 and the f32 round trip
    assert float(dy.abs().max()) == 2.0 and float(x.abs().max()) == 3.0
    assert float(((dy * 4).frac().abs().max())) == 0 and float(((x * 4).frac().abs().max())) == 0
    assert float((want * 16).frac().abs().max()) == 0 and float(want.abs().max()) * 16 <= 96 * largest
    assert want.shape == (320, 192) and torch.equal(want, dy.t() @ x)
    T.assert_exact_range(2 ** 24 // 96)
    with pytest.raises(AssertionError):
        T.assert_exact_range(2 ** 24 // 96 + 1)
    with pytest.raises(AssertionError):
        T.exact_product(dy + 2.0 ** -9, x)                            # not a bf16 value any more
    for M, N, K in T.SELECTOR:
        for mirror in (False, True):
            dy, x, want = T.selector_problem(M, N, K, mirror)
            sel, other = (x, dy) if mirror else (dy, x)
            assert bool(((sel != 0).sum(1) == 1).all()) and int((sel != 0).sum(0).max()) == 1
            assert set(sel[sel != 0].abs().log2().tolist()) == {-2.0, -1.0, 0.0, 1.0, 2.0}
            rows = want.t() if mirror else want
            assert int((rows != 0).any(1).sum()) == M                # M rows (columns) carry one scaled operand row each
            m = 0
            col = int(sel[m].nonzero())
            assert torch.equal(rows[col], float(sel[m, col]) * other[m])


def test_a_forced_slab_count_cannot_overrun_the_workspace():
    """OCTIC_ROUTE_WGRAD_SLABS above 16: the launcher runs at most the 16 slabs octic_dense_wgrad_workspace_bytes has room for."""
    L = _lib.lib()
    for forced in (17, 40):
        with _knob(forced):
            width, tiles, S, _ = _lib.plan(PLAN, 16448, 1280, 0, 1280, 1280)
            need = L.octic_dense_wgrad_workspace_bytes(16448, 1280, 1280)
            pair = _lib.plan(PLAN, 16448, 3840, 1280, 1280, 3840)
            pair_need = L.octic_dense_wgrad_pair_workspace_bytes(16448, 3840, 1280, 1280)
        assert (width, tiles) == (256, 25) and S <= 16, (forced, S)
        assert need >= tiles * S * 256 * 256 * 4 + 4096, (forced, S, need)
        assert pair[2] <= 16 and pair_need >= pair[1] * pair[2] * 256 * 256 * 4 + 4096, (forced, pair, pair_need)
    with _knob(16):
        assert _lib.plan(PLAN, 16448, 1280, 0, 1280, 1280)[2] == 16   # the cap itself is still reachable
    assert _lib.plan(PLAN, 16448, 1280, 0, 1280, 1280)[2] == 8        # and the automatic choice is what it was


def test_the_wide_path_refuses_a_row_stride_shorter_than_the_row():
    """ld < N or K (ld = 0 included) is OCTIC_ESHAPE on the wide path as on the narrow one, before the alignment check and so
    before any launch: dY is passed 2 bytes off, which is as far as an accepted problem gets here."""
    L = _lib.lib()
    p, off = 4096, 4098
    for N, K in ((256, 256), (256, 320), (512, 1280), (128, 64)):
        for ldy, ldx in ((N - 8, K), (N, K - 8), (0, K), (N, 0), (0, 0), (8, 8)):
            assert L.octic_dense_wgrad_tn(off, p, 2056, N, K, ldy, ldx, p, p, None) == ESHAPE, (N, K, ldy, ldx)
            assert L.octic_dense_wgrad_tn_skip(off, p, 2056, N, K, ldy, ldx, p, None, 0, p, None) == ESHAPE, (N, K, ldy, ldx)
        assert L.octic_dense_wgrad_tn(off, p, 2056, N, K, N, K, p, p, None) == EALIGN          # ld == N, K is a row
        assert L.octic_dense_wgrad_tn(off, p, 2056, N, K, N + 8, 3 * K + 16, p, p, None) == EALIGN
    N0, N1, K = 768, 256, 256
    ok = [N0, K, N1, K]
    pair = lambda lds: L.octic_dense_wgrad_tn_pair(off, p, N0, lds[0], lds[1], p, p, p, N1, lds[2], lds[3], p, 2056, K, p, None)
    assert pair(ok) == EALIGN
    for i in range(4):
        for short in (ok[i] - 8, 0):
            assert pair(ok[:i] + [short] + ok[i + 1:]) == ESHAPE, (i, short)
    assert _lib.plan(PLAN, 2056, 256, 0, 256, 248) == (256, 1, 16, 0)   # the plan query asks about the largest stride only


def test_refusals_that_come_back_before_any_launch():
    """Today's refusals, pinned: a pointer off 16 bytes, ld % 8, M % rows_per_sample, a misaligned mask - on the narrow path, both
    wide tiles and the pair.  Every call carries a second flaw that stops it later, so a lost check cannot become a launch."""
    L = _lib.lib()
    p, ss = 4096, 8192
    for N, K in ((256, 256), (256, 320), (128, 64)):
        one = lambda dy, x, dw, ldy=N, ldx=K, M=2056, s=None, rps=0: L.octic_dense_wgrad_tn_skip(dy, x, M, N, K, ldy, ldx, dw, s, rps, p, None)
        for shift in (2, 4, 8):
            assert one(p + shift, p, p) == EALIGN and one(p, p + shift, p) == EALIGN and one(p, p, p + shift) == EALIGN
        for ld_off in (4, 12):                                        # (pointers off as well: ESHAPE comes first)
            assert one(p + 2, p, p, ldy=N + ld_off) == ESHAPE and one(p + 2, p, p, ldx=K + ld_off) == ESHAPE
        assert one(p + 2, p, p, s=ss, rps=256) == ESHAPE and one(p + 2, p, p, s=ss, rps=0) == ESHAPE      # 2056 = 8 x 257
        assert one(p + 2, p, p, s=ss, rps=257) == EALIGN              # (a mask that passes: on to the pointers)
        assert one(p, p, p, ldy=N + 4, s=ss + 2, rps=257) == EALIGN   # the mask is looked at before the strides
        assert one(p, p, p, ldy=N + 4, s=ss, rps=257) == ESHAPE
    N0, N1, K = 768, 256, 256
    two = lambda ptrs, lds, s=None, rps=0: L.octic_dense_wgrad_tn_pair_skip(ptrs[0], ptrs[1], N0, lds[0], lds[1], ptrs[2], ptrs[3], ptrs[4],
                                                                         N1, lds[2], lds[3], ptrs[5], 2056, K, s, rps, p, None)
    ok = [N0, K, N1, K]
    for i in range(6):
        assert two([p + 8 * (j == i) for j in range(6)], ok) == EALIGN, i
    for i in range(4):
        assert two([p + 2] + [p] * 5, ok[:i] + [ok[i] + 4] + ok[i + 1:]) == ESHAPE, i
    assert two([p + 2] + [p] * 5, ok, ss, 256) == ESHAPE
    assert two([p] * 6, [N0 + 4, K, N1, K], ss + 2, 257) == EALIGN
    assert two([p] * 6, [N0 + 4, K, N1, K], ss, 257) == ESHAPE
