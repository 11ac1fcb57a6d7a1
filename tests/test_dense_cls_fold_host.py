"""CPU-only side of octic_dense_gemm_nt_tokens_adaptive_cls (csrc/dense_gemm.hip dense_nt_adaptive_cls_kernel): the adaptive
launch of a masked N = 1280 GEMM with the launch's class-token rows computed by workgroups at the END of its grid.  Which
launches it takes comes through octic_dense_gemm_plan_adaptive_cls, what each workgroup gets through
octic_dense_gemm_order_adaptive_cls (the kernel's own mapping functions run on the host).

The tile workgroups are compared with octic_dense_gemm_order_adaptive, which was there before; the class-token items with the
tiling built here: range(ceil(B / 16)) x range(N // 16), each exactly once."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

from octic_vits_amd import _lib

TOK = 257
NEW = ("octic_dense_gemm_nt_tokens_adaptive_cls", "octic_dense_gemm_plan_adaptive_cls", "octic_dense_gemm_order_adaptive_cls")


@contextlib.contextmanager
def routed(tile=0, image=0, split=0):
    """split = 1: nothing split along K (a long K at a small batch would be: the plan sees a partial round)."""
    try:
        _lib.route_override(_lib.ROUTE_DENSE_TILE, tile)
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, image)
        _lib.route_override(_lib.ROUTE_DENSE_SPLIT, split)
        yield
    finally:
        _lib.route_override(_lib.ROUTE_DENSE_TILE, 0)
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, 0)
        _lib.route_override(_lib.ROUTE_DENSE_SPLIT, 0)


def plan_fold(B, N, K, mode=0, tokens=TOK, rps=TOK):
    out = (ctypes.c_int * 5)()
    assert _lib.lib().octic_dense_gemm_plan_adaptive_cls(B * TOK, N, K, mode, tokens, rps, out) == 0
    return tuple(out)


def plan_adaptive(B, N, K, mode=0, tokens=TOK, rps=TOK):
    out = (ctypes.c_int * 5)()
    assert _lib.lib().octic_dense_gemm_plan_adaptive(B * TOK, N, K, mode, tokens, rps, out) == 0
    return tuple(out)


def scales(keep):
    return np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)


def order_adaptive(B, N, K, keep, cap=4096):
    sc = scales(keep)
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(3)]
    width = ctypes.c_int(-7)
    g = _lib.lib().octic_dense_gemm_order_adaptive(B * TOK, N, K, 0, TOK, sc.ctypes.data, TOK, cap, *[a.ctypes.data for a in arrs],
                                                   ctypes.addressof(width))
    assert g > 0, g
    return [a[:g].tolist() for a in arrs] + [width.value]


def order_fold(B, N, K, keep, cap=4096, cls_cap=4096):
    """-> (tm, tn, dead, width) of the tile workgroups, (tm, tn, dead) of the class-token workgroups, their items per workgroup"""
    sc = scales(keep)
    taken, grid, wgs, per_wg, tile_wgs = plan_fold(B, N, K)
    assert taken == 1 and grid == tile_wgs + wgs
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(3)]
    cls = [np.full(cls_cap, -7, dtype=np.int32) for _ in range(2)]
    width = ctypes.c_int(-7)
    g = _lib.lib().octic_dense_gemm_order_adaptive_cls(B * TOK, N, K, 0, TOK, sc.ctypes.data, TOK, cap, *[a.ctypes.data for a in arrs],
                                                       ctypes.addressof(width), cls_cap, *[a.ctypes.data for a in cls])
    assert g == grid, (g, grid)
    assert all(bool((a[g:] == -7).all()) for a in arrs) and all(bool((a[wgs * per_wg:] == -7).all()) for a in cls)
    tiles = [a[:tile_wgs].tolist() for a in arrs] + [width.value]
    tail = [a[tile_wgs:g].tolist() for a in arrs]
    items = [list(zip(cls[0][w * per_wg:(w + 1) * per_wg].tolist(), cls[1][w * per_wg:(w + 1) * per_wg].tolist())) for w in range(wgs)]
    return tiles, tail, items


def check_fold(B, N, K, keep):
    tiles, tail, items = order_fold(B, N, K, keep)
    assert tiles == order_adaptive(B, N, K, keep), "the tile workgroups are not the adaptive launch's, workgroup by workgroup"
    # the class-token workgroups hold no tile: they sit behind every tile workgroup, none in front
    assert all(t == -1 for t in tail[0]) and all(t == -1 for t in tail[1]) and not any(tail[2])
    flat = [it for w in items for it in w if it != (-1, -1)]
    assert all(rt >= 0 and ct >= 0 for rt, ct in flat)
    assert sorted(flat) == [(r, c) for r in range(-(-B // 16)) for c in range(N // 16)], "a class-token item twice or missing"
    assert all(any(it != (-1, -1) for it in w) for w in items), "a class-token workgroup without work"
    return items


def test_eligibility():
    """Taken: the adaptive launch's eligibility and a K of at most 16 slices of 320."""
    for K in (640, 1280, 3840, 5120):
        assert plan_adaptive(64, 1280, K)[0] == 1, K
        taken, grid, wgs, per_wg, tile_wgs = plan_fold(64, 1280, K)
        assert (taken, tile_wgs) == (1, 320) and grid == 320 + wgs and 0 < wgs <= 96, K
        assert wgs * per_wg >= 320                                   # 4 x 80 class-token items
    # a class-token workgroup outlives no live tile at K = 1280 with 96 free CUs: at most two passes of two items each, all on
    # free CUs at once
    assert plan_fold(64, 1280, 1280)[2:4] == (80, 4)
    assert plan_fold(64, 1280, 640)[2:4] == (80, 4)                  # one pass of four items
    assert plan_fold(64, 1280, 5120)[2:4] == (80, 4)                 # four passes of one item
    for K in (128, 960):
        assert plan_fold(64, 1280, K)[0] == 0, K
        assert plan_fold(64, 1280, K)[2] == 0
    assert plan_fold(64, 1280, 1280, tokens=0)[0] == 0               # classic panels: not the adaptive launch
    assert plan_fold(64, 1280, 1280, mode=4)[0] == 0                 # a fused tail
    assert plan_fold(64, 1280, 1280, mode=2)[0] == 0                 # the unmasked launch (mode 2 takes no mask)
    assert plan_fold(64, 640, 1280)[0] == 0                          # 256 does not divide N
    L = _lib.lib()
    out = (ctypes.c_int * 5)()
    assert L.octic_dense_gemm_plan_adaptive_cls(64 * TOK, 1280, 1280, 0, TOK, 0, out) == -1
    assert L.octic_dense_gemm_plan_adaptive_cls(64 * TOK, 1280, 1280, 0, TOK, TOK, None) == -4
    sc = np.ones(64, dtype=np.float32)
    q = lambda K, s=sc.ctypes.data, cap=4096: L.octic_dense_gemm_order_adaptive_cls(64 * TOK, 1280, K, 0, TOK, s, TOK, cap, None, None,
                                                                                   None, None, 0, None, None)
    assert q(1280) == 400 and q(128) == -1 and q(1280, cap=399) == -1 and q(1280, s=None) == -4
    buf = np.zeros(16, dtype=np.int32)
    assert L.octic_dense_gemm_order_adaptive_cls(64 * TOK, 1280, 1280, 0, TOK, sc.ctypes.data, TOK, 4096, None, None, None, None, 16,
                                                 buf.ctypes.data, None) == -1


@pytest.mark.parametrize("B", range(1, 9))
def test_every_mask_of_small_batches(B):
    """All 2^B masks, K 640 (per-image panels and the 320-wide plan forced: the model would not choose them this small), by the
    rule and under both forced widths."""
    N, K = 1280, 640
    for force in (0, _lib.DENSE_ADAPT_WIDE, _lib.DENSE_ADAPT_NARROW):
        with routed(tile=5 + force, image=1):
            assert plan_fold(B, N, K)[0] == 1 and plan_fold(B, N, K)[4] == 5 * B
            for bits in itertools.product((0, 1), repeat=B):
                check_fold(B, N, K, list(bits))


def test_seeded_masks_at_64_images():
    """500 seeded masks at the headline shape with 38 / 39 (64 CUs free or not) and 51 / 52 kept (narrow or wide) forced in."""
    B, N = 64, 1280
    rng = np.random.default_rng(320 + 80)
    forced = (38, 39, 51, 52)
    seen = set()
    for i in range(500):
        keep = (rng.random(B) < (0.5, 0.6, 0.8, rng.random())[i % 4]).tolist()
        if i % 8 == 1:
            n = forced[(i // 8) % 4]
            keep = [True] * n + [False] * (B - n)
            rng.shuffle(keep)
        seen.add(sum(keep))
        check_fold(B, N, (640, 1280, 3840, 5120)[i % 4], keep)
    assert set(forced) <= seen


@pytest.mark.parametrize("K", (320, 640, 960, 1280, 1920, 2560, 3200, 3840, 5120))
def test_items_of_every_slice_count(K):
    """Slices 2 .. 16: items per pass 4 / 2 / 1 ... - every item once, passes dealt grid-stride (workgroup w takes the
    items of passes w, w + C, ...)."""
    B, N = 19, 1280
    with routed(tile=5, image=1, split=1):
        if K % 128:
            assert plan_fold(B, N, K)[0] == 0                        # no per-image panels: the class-token kernels need K % 128 == 0
            return
        items = check_fold(B, N, K, [1, 0] * 9 + [1])
        wgs, per_wg = plan_fold(B, N, K)[2:4]
    nks = K // 320
    ipp = 8 // nks if nks <= 8 else 1
    ntn = N // 16
    for w, its in enumerate(items):
        for e, it in enumerate(its):
            item = ((e // ipp) * wgs + w) * ipp + e % ipp
            assert it == ((item // ntn, item % ntn) if item < 2 * ntn else (-1, -1))


def test_new_entry_points_are_declared_prototyped_and_exported():
    L = _lib.lib()
    assert set(NEW) <= set(_lib.header_symbols()) and set(NEW) <= set(_lib._PROTOS)
    for name in NEW:
        assert hasattr(L, name)
    a, c = (list(_lib._PROTOS[n][1]) for n in ("octic_dense_gemm_nt_tokens_adaptive", "octic_dense_gemm_nt_tokens_adaptive_cls"))
    assert c == a[:-1] + [ctypes.c_int, a[-1]]                       # fold_cls in front of the stream
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20           # additions only


def test_launch_refusals_come_back_before_any_launch():
    L = _lib.lib()
    p, ss = 4096, 8192
    f = lambda M, s, rps, a=p: L.octic_dense_gemm_nt_tokens_adaptive_cls(a, p, M, 1280, 640, 640, 640, 0, p, None, 1280, None, None,
                                                                         None, 1, None, None, None, None, s, rps, p, TOK, 1, None)
    assert f(771, ss, 0) == -1 and f(771, ss, 256) == -1 and f(771, ss + 2, 257) == -2 and f(771, ss, 257, a=None) == -4


def test_switch_and_threshold(monkeypatch):
    import octic_vits_amd.functional as OF
    from octic_vits_amd import ops
    monkeypatch.delenv("OCTIC_DENSE_CLS_FOLD", raising=False)
    assert OF._skip_from_env("OCTIC_DENSE_CLS_FOLD") is True         # on by default
    monkeypatch.setenv("OCTIC_DENSE_CLS_FOLD", "0")
    assert OF._skip_from_env("OCTIC_DENSE_CLS_FOLD") is False
    monkeypatch.setattr(OF, "DENSE_CLS_FOLD", True)
    monkeypatch.setattr(OF, "DENSE_NARROW_DROPPED", True)
    assert OF.DENSE_CLS_FOLD_MIN_DROP == 0.4
    assert OF.dense_cls_fold(0.5) and OF.dense_cls_fold(0.4) and not OF.dense_cls_fold(0.39) and not OF.dense_cls_fold(None)
    assert ops._dense_cls_fold() is True
    monkeypatch.setattr(OF, "DENSE_NARROW_DROPPED", False)           # effective only while the adaptive launch is on
    assert not OF.dense_cls_fold(0.5) and ops._dense_cls_fold() is False
    monkeypatch.setattr(OF, "DENSE_NARROW_DROPPED", True)
    monkeypatch.setattr(OF, "DENSE_CLS_FOLD", False)
    assert not OF.dense_cls_fold(0.5) and ops._dense_cls_fold() is False
    assert ops.dense_plan_adaptive_cls(64 * TOK, 1280, 1280, 0, TOK, TOK) == (True, 400, 80, 4, 320)
