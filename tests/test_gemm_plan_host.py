"""Which kernel a GEMM shape runs: the library's three plan queries - octic_linear_d8_plan (linear_plan, csrc/gemm.hip),
octic_linear_d8_wgrad_plan (wgrad_plan, csrc/wgrad.hip) and octic_dense_wgrad_plan (dw_route, csrc/dense_wgrad.hip), the
functions the entry points launch from - against the rules written out below, and ops.dense_wgrad_ok / dense_wgrad_pair_ok
against the formulas they had as hand-kept copies.  No GPU needed (without a device the library counts 256 CUs).

The expected tables were built from the code paths of the commit before the plans existed (launch_t's refusals, ring_ok,
launch_ring's wide-tile test, pick_nt, wgrad_ring_ok, pick_tt, octic_linear_d8_wgrad_splits, the four TN entry points); the
library agrees with every cell."""
import ctypes

import pytest

F32, BF16 = 0, 1
WREG, RING, CLASSIC = range(3)                     # OCTIC_LINEAR_*
WG_RING, WG_TILED = range(2)                       # OCTIC_WGRAD_*
ESHAPE, EDTYPE, ENULL = -1, -3, -4
ROWS = (33, 16448)
PAIRS = ((F32, F32), (BF16, BF16), (BF16, F32))


def _step(dtype):
    return 4 if dtype == F32 else 8


def _cins(dtype):
    return range(_step(dtype), 1281, _step(dtype))


def _couts(cin):
    return sorted({cin, 3 * cin, 4 * cin, max(8, cin // 4)})


def _groups(M, cin, cout):
    """The five sub-problems of a launch, E first: (rows, K, N)."""
    return [(2 * M, 2 * cin, 2 * cout)] + [(M, cin, cout)] * 4


def _pick(groups, cost):
    """Least padded work over tile parameters 2 .. 5, the wider tile on (near) ties - pick_nt / pick_tt."""
    best, best_cost = 2, 1e30
    for t in range(2, 6):
        c = sum(cost(32 * t, rows, K, N) for rows, K, N in groups)
        if c <= best_cost * 1.0001:
            best_cost, best = min(c, best_cost), t
    return best


def _ceil(a, b):
    return (a + b - 1) // b


def linear_expected(M, cin, cout, dtype, fused, ring_knob=False):
    """(kernel, columns per output tile, fused instantiation, 0) of octic_linear_d8_plan."""
    if dtype == BF16 and cin % 32 == 0 and 32 <= cin <= 160 and not ring_knob:
        return WREG, 0, fused, 0
    if cin % (32 if dtype == BF16 else 16) == 0:
        wide = dtype == BF16 and cout % 160 == 0 and cin >= 2 * cout
        return RING, 160 if wide else 80, fused, 0
    nt = _pick(_groups(M, cin, cout), lambda bn, rows, K, N: float(_ceil(N, bn)) * bn * float(K) * float(rows))
    return CLASSIC, 32 * nt, 0, 0


def wgrad_expected(M, cin, cout, dtype):
    """(kernel, tile width, splits, has_colsum) of octic_linear_d8_wgrad_plan."""
    ring = dtype == BF16 and cin % 160 == 0 and cout % 160 == 0
    tt = _pick(_groups(M, cin, cout), lambda bw, rows, K, N: float(_ceil(K, bw) * _ceil(N, bw)) * bw * bw * float(rows))
    bw = 32 * tt
    tiles_e = _ceil(2 * cin, bw) * _ceil(2 * cout, bw)
    tiles_1 = 4 * _ceil(cin, bw) * _ceil(cout, bw)
    splits = int(512.0 / (tiles_e + 0.5 * tiles_1) + 0.5)
    splits = max(1, min(splits, (2 * M + 255) // 256, 32))
    return WG_RING if ring else WG_TILED, bw, splits, int(ring)


def _query(name, *args):
    from octic_vits_amd import _lib
    out = (ctypes.c_int * 4)()
    code = getattr(_lib.lib(), name)(*args, out)
    return tuple(out) if code == 0 else code


def _linear_mismatches(ring_knob):
    bad = []
    for dtype, out_dtype in PAIRS:
        for cin in _cins(dtype):
            for cout in _couts(cin):
                legal = cout % _step(dtype) == 0 and cout % _step(out_dtype) == 0
                for M in ROWS:
                    for fused in (0, 1):
                        got = _query("octic_linear_d8_plan", M, cin, cout, dtype, out_dtype, fused)
                        want = linear_expected(M, cin, cout, dtype, fused, ring_knob) if legal else ESHAPE
                        if got != want:
                            bad.append((dtype, out_dtype, M, cin, cout, fused, got, want))
    return bad


def test_ids_match_the_header():
    import re
    from octic_vits_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    for name, value in (("LINEAR_WREG", WREG), ("LINEAR_RING", RING), ("LINEAR_CLASSIC", CLASSIC), ("WGRAD_RING", WG_RING),
                        ("WGRAD_TILED", WG_TILED)):
        assert int(re.search(r"OCTIC_%s = (\d+)" % name, text).group(1)) == value == getattr(_lib, name), name
    assert int(re.search(r"#define OCTIC_ABI_VERSION (\d+)", text).group(1)) == 20 == _lib.ABI_VERSION


def test_linear_plan_matches_the_rules_at_every_legal_width():
    bad = _linear_mismatches(ring_knob=False)
    assert not bad, (len(bad), bad[:8])


def test_linear_plan_under_the_ring_knob_never_says_w_stationary():
    from octic_vits_amd import _lib
    try:
        assert _lib.route_override(_lib.ROUTE_LINEAR_RING, 1) == 0
        bad = _linear_mismatches(ring_knob=True)
        kernels = {_query("octic_linear_d8_plan", M, cin, cin, BF16, BF16, 0)[0] for cin in _cins(BF16) for M in ROWS}
    finally:
        _lib.route_override(_lib.ROUTE_LINEAR_RING, 0)
    assert not bad, (len(bad), bad[:8])
    assert kernels == {RING, CLASSIC}
    assert _query("octic_linear_d8_plan", 96, 32, 32, BF16, BF16, 0) == (WREG, 0, 0, 0)      # the knob is back at 0


def test_the_rules_reach_every_branch():
    """(a table that never said W-stationary, wide or classic would let a dead branch pass)"""
    assert linear_expected(16448, 160, 480, BF16, 1) == (WREG, 0, 1, 0)
    assert linear_expected(16448, 160, 480, BF16, 1, ring_knob=True) == (RING, 80, 1, 0)
    assert linear_expected(16448, 640, 160, BF16, 0) == (RING, 160, 0, 0) and linear_expected(16448, 320, 320, BF16, 0)[1] == 80
    assert linear_expected(16448, 640, 160, F32, 0) == (RING, 80, 0, 0)
    assert linear_expected(64, 24, 24, F32, 1) == (CLASSIC, 64, 0, 0) and linear_expected(64, 32, 24, F32, 0)[0] == RING
    classic = {linear_expected(33, cin, cout, BF16, 0) for cin in _cins(BF16) for cout in _couts(cin)}
    assert {tile for kernel, tile, _, _ in classic if kernel == CLASSIC} == {64, 96, 128, 160}
    assert wgrad_expected(257, 160, 160, BF16) == (WG_RING, 160, 3, 1) and wgrad_expected(257, 160, 160, F32)[0] == WG_TILED
    assert {wgrad_expected(16448, cin, cin, BF16)[1] for cin in _cins(BF16)} == {64, 96, 128, 160}
    assert {wgrad_expected(M, cin, cin, BF16)[2] for cin in _cins(BF16) for M in ROWS} >= {1, 2, 32}


def test_linear_plan_refuses_what_the_entry_point_refuses():
    for cin in (8, 32, 160, 168, 640):
        assert _query("octic_linear_d8_plan", 33, cin, cin, F32, BF16, 0) == EDTYPE
    assert _query("octic_linear_d8_plan", 0, 32, 32, BF16, BF16, 0) == ESHAPE
    assert _query("octic_linear_d8_plan", 33, 36, 32, BF16, BF16, 0) == ESHAPE and _query("octic_linear_d8_plan", 33, 36, 32, F32, F32, 0)[0] == CLASSIC
    from octic_vits_amd import _lib
    assert _lib.lib().octic_linear_d8_plan(33, 32, 32, BF16, BF16, 0, None) == ENULL
    assert _lib.lib().octic_linear_d8_wgrad_plan(33, 32, 32, BF16, None) == ENULL
    assert _lib.lib().octic_dense_wgrad_plan(33, 256, 0, 256, 0, None) == ENULL


@pytest.mark.parametrize("dtype", (BF16, F32))
def test_wgrad_plan_matches_the_rules_and_the_single_answer_queries(dtype):
    from octic_vits_amd import _lib
    L = _lib.lib()
    bad = []
    for cin in _cins(dtype):
        for cout in _couts(cin):
            for M in ROWS:
                got = _query("octic_linear_d8_wgrad_plan", M, cin, cout, dtype)
                if cout % _step(dtype):
                    ok = got == ESHAPE
                else:
                    old = (L.octic_linear_d8_wgrad_tile(M, cin, cout), L.octic_linear_d8_wgrad_splits(M, cin, cout),
                           L.octic_linear_d8_wgrad_has_colsum(cin, cout, dtype))
                    ok = got == wgrad_expected(M, cin, cout, dtype) and old == got[1:]
                if not ok:
                    bad.append((M, cin, cout, got))
    assert not bad, (len(bad), bad[:8])


# ---- dense TN weight gradient --------------------------------------------------------------------------------------------

def _tn_tile(M, N, K):
    """Tile width of octic_dense_wgrad_tn by shape alone: 256 | 320 where the wide tiles divide N x K, 64 on the narrow path."""
    if M <= 0:
        return 0
    if N % 256 == 0 and (K % 256 == 0 or K % 320 == 0):
        return 256 if K % 256 == 0 else 320
    return 64 if N % 64 == 0 and K % 64 == 0 else 0


def _old_wgrad_ok(M, N, K):
    wide = N % 256 == 0 and (K % 256 == 0 or K % 320 == 0)
    narrow = N % 64 == 0 and K % 64 == 0 and not wide
    return M > 0 and ((wide and (N // 256) * (K // 256) <= 256) or narrow)


def _old_wgrad_pair_ok(M, N0, N1, K):
    return (N0 % 256 == 0 and N1 % 256 == 0 and (K % 256 == 0 or K % 320 == 0) and M > 0
            and ((N0 + N1) // 256) * (K // 256) <= 256)


def test_dense_wgrad_ok_is_the_plan_and_the_cap():
    from octic_vits_amd import _lib, ops
    L = _lib.lib()
    bad, capped = [], 0
    for M in (1, 257, 16448):
        for N in range(64, 5185, 64):
            for K in range(64, 5185, 64):
                plan = _query("octic_dense_wgrad_plan", M, N, 0, K, 0)
                tile = L.octic_dense_wgrad_tile(M, N, K)
                ok = ops.dense_wgrad_ok(M, N, K)
                capped += tile != 0 and not ok
                if not (ok is _old_wgrad_ok(M, N, K) and tile == _tn_tile(M, N, K) and (plan[0] if tile else plan) == (tile or ESHAPE)):
                    bad.append((M, N, K, ok, tile, plan))
    _lib._PLANS.clear()
    assert not bad, (len(bad), bad[:8])
    assert capped == 156                              # the shapes the library takes and the routing cap of ops.py keeps out


def test_dense_wgrad_pair_ok_is_the_plan_and_the_cap():
    from octic_vits_amd import _lib, ops
    bad = []
    for M in (1, 16448):
        for N0 in range(256, 3841, 256):
            for N1 in range(256, 3841, 256):
                for K in range(256, 5121, 64):
                    plan = _query("octic_dense_wgrad_plan", M, N0, N1, K, 0)
                    wide = K % 256 == 0 or K % 320 == 0
                    want_plan = plan != ESHAPE and plan[0] == _tn_tile(M, N0 + N1, K) if wide else plan == ESHAPE
                    if not (ops.dense_wgrad_pair_ok(M, N0, N1, K) is _old_wgrad_pair_ok(M, N0, N1, K) and want_plan):
                        bad.append((M, N0, N1, K, plan))
    _lib._PLANS.clear()
    assert not bad, (len(bad), bad[:8])
    for args in ((16448, 256, 64, 256), (16448, 64, 256, 256), (16448, 192, 192, 192), (0, 256, 256, 256), (16448, 256, -256, 256)):
        assert _query("octic_dense_wgrad_plan", *args, 0) == ESHAPE and not ops.dense_wgrad_pair_ok(*args), args
    assert ops.dense_wgrad_pair_ok(16448, 3840, 1280, 1280) and not ops.dense_wgrad_pair_ok(16448, 3840, 0, 1280)


def test_dense_wgrad_plan_counts_tiles_and_slabs():
    """256 CUs without a device: 5120 x 1280 is 100 tiles in 2 slabs, 1280 x 1280 25 tiles (32 with padding) in 8, the 320-wide tile
    serves K % 320 == 0 only, 384 x 384 takes the narrow path; more than 1024 tiles is refused."""
    assert _query("octic_dense_wgrad_plan", 16448, 5120, 0, 1280, 1280) == (256, 100, 2, 0)
    assert _query("octic_dense_wgrad_plan", 16448, 1280, 0, 1280, 1280) == (256, 25, 8, 0)
    assert _query("octic_dense_wgrad_plan", 16448, 3840, 1280, 1280, 3840) == (256, 100, 2, 0)
    assert _query("octic_dense_wgrad_plan", 16448, 1280, 0, 960, 1280)[:2] == (320, 15)
    assert _query("octic_dense_wgrad_plan", 16448, 384, 0, 384, 384) == (64, 36, 15, 0)
    assert _query("octic_dense_wgrad_plan", 16448, 8192, 0, 8192, 0)[1] == 1024
    assert _query("octic_dense_wgrad_plan", 16448, 8448, 0, 8192, 0) == ESHAPE


def test_strides_beyond_32_bit_offsets_are_refused_on_the_wide_path():
    """M * ld * 2 >= 2^31 is past the 32-bit buffer offsets of dense_tn_kernel; the narrow kernel addresses with 64 bits."""
    from octic_vits_amd import ops
    M, inside, beyond = 16448, 65280, 65281
    assert M * beyond * 2 >= 2 ** 31 > M * inside * 2
    assert _query("octic_dense_wgrad_plan", M, 1280, 0, 1280, inside) == (256, 25, 8, 0)
    assert _query("octic_dense_wgrad_plan", M, 1280, 0, 1280, beyond) == ESHAPE
    assert _query("octic_dense_wgrad_plan", M, 3840, 1280, 1280, inside) != ESHAPE
    assert _query("octic_dense_wgrad_plan", M, 3840, 1280, 1280, beyond) == ESHAPE
    assert ops.dense_wgrad_ok(M, 1280, 1280, inside) and not ops.dense_wgrad_ok(M, 1280, 1280, beyond)
    assert _query("octic_dense_wgrad_plan", M, 384, 0, 384, beyond) == (64, 36, 15, 0)


def test_tn_entry_points_refuse_what_the_plan_refuses():
    """One refusal: a shape or stride is OCTIC_ESHAPE for octic_dense_wgrad_plan exactly where it is for the launchers (checked
    before any launch, so no GPU is touched): a misaligned dY gets a shape the plan takes as far as the alignment check (-2)."""
    from octic_vits_amd import _lib
    L = _lib.lib()
    p = 4096
    for M, N, K, ld in ((16448, 1280, 1280, 1280), (16448, 1280, 1280, 65288), (16448, 1280, 960, 1280), (16448, 384, 384, 384),
                        (16448, 1280, 1344, 1344), (16448, 8448, 8192, 8448), (0, 256, 256, 256), (16448, 200, 256, 256)):
        want = _query("octic_dense_wgrad_plan", M, N, 0, K, ld)
        got = L.octic_dense_wgrad_tn(p + 2, p, M, N, K, ld, ld, p, p, None)
        assert (want != ESHAPE, got) in ((True, -2), (False, ESHAPE)), (M, N, K, ld, want, got)
        assert (L.octic_dense_wgrad_tile(M, N, K) != 0) == (_query("octic_dense_wgrad_plan", M, N, 0, K, 0) != ESHAPE)
    for M, N0, N1, K, ld in ((16448, 3840, 1280, 1280, 3840), (16448, 3840, 1280, 1280, 65288), (16448, 3840, 1280, 1344, 3840),
                             (16448, 3840, 192, 1280, 3840), (16448, 8448, 256, 8192, 8704)):
        want = _query("octic_dense_wgrad_plan", M, N0, N1, K, ld)
        got = L.octic_dense_wgrad_tn_pair(p + 2, p, N0, ld, ld, p, p, p, N1, ld, ld, p, M, K, p, None)
        assert (want != ESHAPE, got) in ((True, -2), (False, ESHAPE)), (M, N0, N1, K, ld, want, got)
