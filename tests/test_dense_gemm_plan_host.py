"""octic_dense_gemm_plan / octic_dense_gemm_workspace_bytes under OCTIC_ROUTE_DENSE_SPLIT, and the workspace cache of
ops.dense_gemm_nt: host arithmetic, no GPU needed (without a device the library counts 256 CUs).

The hazard these tests pin down: ops._dense_ws caches the split-K workspace of an (M, N, K) at the size the library states
when the shape first runs - 256 bytes where the plan splits nothing.  A launch planned under a forced split needs tickets and
slabs; _lib.route_override therefore drops the cached workspaces together with the cached plans."""
import ctypes

import pytest

ESHAPE, ENULL = -1, -4
TICKETS = 8192                                     # DG_TICKET_BYTES: the ticket words in front of the slabs
CUS = 256


def _plan(M, N, K, mode=0, tokens=0):
    from octic_vits_amd import _lib
    out = (ctypes.c_int * 4)()
    assert _lib.lib().octic_dense_gemm_plan(M, N, K, mode, tokens, out) == 0
    return tuple(out)


def _bytes(M, N, K):
    from octic_vits_amd import _lib
    return int(_lib.lib().octic_dense_gemm_workspace_bytes(M, N, K))


def _split(value):
    from octic_vits_amd import _lib
    return _lib.route_override(_lib.ROUTE_DENSE_SPLIT, value)


def test_route_override_drops_the_cached_dense_workspaces():
    from octic_vits_amd import _lib, ops
    ops._DG_WS[(300, 264, 1024, "nowhere")] = object()
    _lib.plan("octic_dense_gemm_plan", 300, 264, 1024, 0, 0)
    assert ops._DG_WS and _lib._PLANS
    try:
        _split(4)
        assert not ops._DG_WS and not _lib._PLANS
        ops._DG_WS[(300, 264, 1024, "nowhere")] = object()
    finally:
        _split(0)
    assert not ops._DG_WS                           # ... and again on the way back: neither table's sizes outlive it
    # any knob, not only the split: the override table is one thing
    ops._DG_WS[(1, 1, 1, "nowhere")] = object()
    _lib.route_override(_lib.ROUTE_DENSE_IMAGE, 0)
    assert not ops._DG_WS


def test_the_drop_is_registered_once_and_no_plan_query_is_added_per_launch():
    from octic_vits_amd import _lib, ops
    assert _lib._ON_OVERRIDE.count(ops._DG_WS.clear) == 1
    assert _lib.on_route_override(ops._DG_WS.clear) is not None and _lib._ON_OVERRIDE.count(ops._DG_WS.clear) == 1


def test_workspace_bytes_follow_the_split_knob():
    """300 x 264 x 512: 2 x 2 tiles of 8 K-tiles - the model leaves them unsplit (256 bytes: nothing is ever written), a
    forced split needs the ticket words and rem * split slabs of 256 x 256 f32."""
    M, N, K = 300, 264, 512
    rem, smax = 4, K // 64 // 4
    try:
        assert _split(0) == 0
        assert _bytes(M, N, K) == 256
        assert _split(2) == 0
        assert _bytes(M, N, K) >= TICKETS + rem * min(2, smax) * 256 * 256 * 4
    finally:
        _split(0)
    assert _bytes(M, N, K) == 256


def test_workspace_bytes_of_the_issue_shape():
    """300 x 264 x 1024 (16 K-tiles): with the knob at 4 there is room for 4 tiles x 4 parts.  With the knob at 0 the launch
    model splits this shape four ways by itself (16 / 4 + 17 x 0.586 + 1 < 16 K-tiles), so its workspace is the same size,
    not 256 bytes - what must hold is that the bytes cover the plan in force, whichever table it was made under."""
    M, N, K = 300, 264, 1024
    need4 = TICKETS + 4 * 4 * 256 * 256 * 4
    try:
        _split(4)
        assert _plan(M, N, K)[3] == 16 and _bytes(M, N, K) >= need4
    finally:
        _split(0)
    natural = (_plan(M, N, K)[3] // 4)              # parts per tile of the model's own plan (grid = 4 tiles x parts, padded to 8)
    assert _bytes(M, N, K) >= (TICKETS + 4 * natural * 256 * 256 * 4 if natural > 1 else 256)


@pytest.mark.parametrize("M,N,K", [(300, 264, 512), (300, 264, 1280), (300, 264, 2048), (257, 264, 1280), (300, 520, 1024),
                                   (771, 272, 768)])
@pytest.mark.parametrize("s", (2, 3, 4, 5, 8))
def test_forced_split_grid(M, N, K, s):
    """Fewer tiles than CUs: every tile is cut min(s, K / 64 / 4) ways (at least four K-tiles per part), the parts are padded
    to a multiple of 8 workgroups; the workspace holds them."""
    tiles = -(-M // 256) * -(-N // 256)
    assert tiles < CUS
    parts = min(s, K // 64 // 4)
    try:
        _split(s)
        for mode in range(7):
            assert _plan(M, N, K, mode)[3] == (tiles * parts + 7) & ~7, (mode, _plan(M, N, K, mode))
        assert _bytes(M, N, K) >= TICKETS + tiles * parts * 256 * 256 * 4
    finally:
        _split(0)


def test_forced_split_grid_on_the_320_wide_tile():
    from octic_vits_amd import _lib
    try:
        _split(5)
        for nt, width in ((5, 320), (4, 256)):
            _lib.route_override(_lib.ROUTE_DENSE_TILE, nt)
            for N in (320, 640):
                tiles = 2 * -(-N // width)
                assert _plan(300, N, 1280) == (width, 4, 0, (tiles * 5 + 7) & ~7)
                assert _bytes(300, N, 1280) >= TICKETS + tiles * 5 * 256 * width * 4
    finally:
        _lib.route_override(_lib.ROUTE_DENSE_TILE, 0)
        _split(0)


def test_knob_at_zero_is_one_workgroup_per_tile_where_the_model_does_not_split():
    """K of 2 .. 8 K-tiles never pays the slab round trip at 300 x 264; 1280 and 2048 do (five and eight parts)."""
    assert _split(0) == 0
    for K in (128, 192, 256, 512):
        assert _plan(300, 264, K)[3] == 4 and _bytes(300, 264, K) == 256, K
    assert _plan(300, 264, 1280)[3] == 24 and _plan(300, 264, 2048)[3] == 32
    assert _plan(3000, 520, 4096)[3] == 256          # 36 tiles cut seven ways


def test_knob_at_one_keeps_a_thin_tail_in_front_without_a_workspace():
    """8212 x 2048 x 128: one round of 256 tiles + the 8 tiles of the 20-row panel.  Unsplit either way - 264 workgroups - and
    no slab is ever written: 256 bytes."""
    try:
        _split(1)
        assert _plan(8212, 2048, 128)[3] == 264 and _bytes(8212, 2048, 128) == 256
    finally:
        _split(0)
    assert _plan(8212, 2048, 128)[3] == 264


def test_entry_point_refuses_a_row_stride_of_c_that_misaligns_its_16_byte_stores():
    """ldc % 8: every epilogue moves 8 bf16 of a row of C / C2 / H per lane.  Refused before any launch (no GPU is touched);
    a legal shape gets as far as the alignment check of A / B (-2)."""
    from octic_vits_amd import _lib
    L = _lib.lib()
    p = 4096

    def call(M, N, K, lda, ldb, ldc, a=p):
        return L.octic_dense_gemm_nt_tokens(a, p, M, N, K, lda, ldb, 0, p, None, ldc, None, None, None, 1, None, None, None, None,
                                            None, 0, None)
    assert call(300, 264, 256, 256, 256, 264, a=p + 2) == -2
    assert call(300, 264, 256, 256, 256, 272, a=p + 2) == -2
    assert call(300, 264, 256, 256, 256, 268) == ESHAPE            # ldc % 4 == 0 but not % 8
    assert call(300, 264, 256, 256, 256, 266) == ESHAPE
    assert call(300, 260, 256, 256, 256, 264) == ESHAPE            # N % 8
    assert call(300, 264, 96, 96, 96, 264) == ESHAPE               # K % 64
    assert call(300, 264, 64, 64, 64, 264) == ESHAPE               # fewer than two K-tiles
    assert call(300, 264, 192, 192, 192, 264, a=p + 2) == -2       # K = 192 is taken
    assert call(300, 264, 256, 260, 256, 264) == ESHAPE            # lda % 8
    assert L.octic_dense_gemm_nt_tokens(None, p, 300, 264, 256, 256, 256, 0, p, None, 264, None, None, None, 1, None, None, None,
                                        None, None, 0, None) == ENULL
