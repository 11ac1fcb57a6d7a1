"""CPU-only side of octic_dense_gemm_nt_tokens_image (csrc/dense_gemm.hip dense_plan_image, dense_nt_image_cls_kernel): which
masked launches leave classic 256-row panels for per-image ones comes through octic_dense_gemm_plan_image, what each workgroup gets
through octic_dense_gemm_order_image (the kernel's own mapping functions run on the host).  256 workgroup slots (no device: the
library plans for 256 CUs)."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

from octic_vits_amd import _lib

TOK = 257
NEW = ("octic_dense_gemm_nt_tokens_image", "octic_dense_gemm_plan_image", "octic_dense_gemm_order_image")
THREE = ((3840, 1280, 0), (5120, 1280, 4), (5120, 1280, 5))          # qkv forward, fc1 + factor, the fc2 input gradient
# The per-launch keep rule (csrc/dense_gemm.hip kDgImageKeep) holds fc1 + factor on classic panels: shorter per-image in the step,
# but the step's state then leaves the accepted distance from the parent's (NOTES.md).  By the model alone the library moves the
# other two; fc1 is asserted legal and taken under OCTIC_ROUTE_DENSE_IMAGE + 4, with the plan the other two get.
KEPT = (THREE[0], THREE[2])
HELD = (THREE[1],)
FIVE = ((1280, 1280, 0), (1280, 5120, 0), (1280, 3840, 0))           # proj / dproj, fc2, dqkv (dfc1 = the first): the N = 1280 launches


@contextlib.contextmanager
def routed(image=0):
    try:
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, image)
        yield
    finally:
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, 0)


def plan_image(B, N, K, mode, drop, masked=1, tokens=TOK, rps=TOK):
    out = (ctypes.c_int * 8)()
    assert _lib.lib().octic_dense_gemm_plan_image(B * TOK, N, K, mode, tokens, rps, masked, drop, out) == 0
    return tuple(out)


def plan_former(B, N, K, mode, tokens=TOK):
    out = (ctypes.c_int * 4)()
    assert _lib.lib().octic_dense_gemm_plan(B * TOK, N, K, mode, tokens, out) == 0
    return tuple(out)                                                 # (width, colsum rows, per-image?, workgroups)


def is_former(B, N, K, mode, got, tokens=TOK):
    width, rows, image, grid = plan_former(B, N, K, mode, tokens)
    return got[0] == 0 and got[2] == 0 and got[3] == 0 and got[5:] == (width, rows, image) and got[4] == grid


def test_the_three_multi_round_launches_go_per_image_at_drop_half():
    for N, K, mode in HELD:
        assert is_former(64, N, K, mode, plan_image(64, N, K, mode, 0.5))
    for N, K, mode in THREE:
        with routed(image=0 if (N, K, mode) in KEPT else _lib.DENSE_IMAGE_ALWAYS):
            taken, grid, wgs, per_wg, tile_wgs, width, rows, image = plan_image(64, N, K, mode, 0.5)
        assert (taken, image, width) == (1, 1, 256), (N, K, mode)
        assert tile_wgs == 64 * (N // 256) and grid == tile_wgs + wgs and 0 < wgs <= 128
        assert wgs * per_wg >= 4 * (N // 16)                          # every class-token item has a place
        assert rows == 2 * 64 + 4                                     # two slab rows per image panel + one per class-token row tile
        assert plan_former(64, N, K, mode)[2] == 0                    # ... where the former call stays on classic panels


def test_no_hint_no_mask_and_the_n1280_launches_keep_todays_plan():
    for N, K, mode in THREE + FIVE:
        assert is_former(64, N, K, mode, plan_image(64, N, K, mode, 0.0)), (N, K, mode)
        assert is_former(64, N, K, mode, plan_image(64, N, K, mode, -1.0)), (N, K, mode)
        assert is_former(64, N, K, mode, plan_image(64, N, K, mode, 0.5, masked=0)), (N, K, mode)
    for N, K, mode in FIVE:
        for drop in (0.1, 0.5, 0.9):
            got = plan_image(64, N, K, mode, drop)
            assert is_former(64, N, K, mode, got) and got[7] == 1, (N, K, drop)       # already per-image, by the adaptive path
    # modes the folded launch has no class-token epilogue for, the fused residual tail, classic tokens, per-row masks
    for mode in (1, 2, 3, 6):
        assert is_former(64, 5120, 1280, mode, plan_image(64, 5120, 1280, mode, 0.5))
    assert is_former(64, 5120, 1280, 5, plan_image(64, 5120, 1280, 5, 0.5, tokens=0), tokens=0)
    assert is_former(64, 5120, 1280, 5, plan_image(64, 5120, 1280, 5, 0.5, rps=1))
    with routed(image=2):
        assert plan_image(64, 5120, 1280, 5, 0.5)[0] == 0
    with routed(image=_lib.DENSE_IMAGE_NEVER):
        assert plan_image(64, 5120, 1280, 5, 0.5)[0] == 0
    with routed(image=_lib.DENSE_IMAGE_NEVER + _lib.DENSE_IMAGE_ALWAYS):
        assert plan_image(64, 5120, 1280, 5, 0.5)[0] == 0


def test_the_choice_is_a_cost_comparison_not_a_shape_list():
    """1 - p^2 against 1 - p: monotone in the drop probability, nothing under one round, other batches and widths follow."""
    for N, K, mode in KEPT:
        taken = [plan_image(64, N, K, mode, p)[0] for p in (0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.7)]
        assert taken == sorted(taken) and taken[0] == 0 and taken[-1] == 1, (N, K, taken)
        assert plan_image(64, N, K, mode, 0.97)[0] == 0               # nearly everything dropped: one round of live tiles either way
    for N, K, mode in HELD:
        assert not any(plan_image(64, N, K, mode, p)[0] for p in (0.02, 0.2, 0.5, 0.7, 0.97))
    assert plan_image(128, 5120, 1280, 5, 0.5)[0] == 1 and plan_image(32, 5120, 1280, 5, 0.5)[0] == 1
    assert plan_image(64, 2560, 1280, 5, 0.5)[0] == 1                 # not a ViT-H width: three rounds classic
    assert plan_image(2, 512, 640, 5, 0.5)[0] == 0 and plan_image(16, 1024, 256, 5, 0.5)[0] == 0     # under one round: one live tile either way
    with routed(image=_lib.DENSE_IMAGE_ALWAYS):
        assert plan_image(2, 512, 640, 4, 0.5)[0] == 1 and plan_image(2, 512, 640, 4, 0.5)[2] > 0
        assert plan_image(2, 512, 640, 1, 0.5)[0] == 0                # ... only launches it can take
    with routed(image=_lib.DENSE_IMAGE_ALWAYS + _lib.DENSE_IMAGE_CLS_APART):
        assert plan_image(2, 512, 640, 4, 0.5)[:5] == (1, 4, 0, 0, 4)
    with routed(image=_lib.DENSE_IMAGE_ALWAYS):
        assert plan_image(2, 512, 384, 4, 0.5)[:5] == (1, 4, 0, 0, 4)  # K is no multiple of 320: the class-token launch


def order(B, N, K, mode, keep, drop=0.5, cap=4096, cls_cap=8192):
    sc = np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)
    taken, grid, wgs, per_wg, tile_wgs = plan_image(B, N, K, mode, drop)[:5]
    assert taken == 1 and grid == tile_wgs + wgs
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(3)]
    cls = [np.full(cls_cap, -7, dtype=np.int32) for _ in range(2)]
    g = _lib.lib().octic_dense_gemm_order_image(B * TOK, N, K, mode, TOK, sc.ctypes.data, TOK, drop, cap, *[a.ctypes.data for a in arrs],
                                                cls_cap, *[a.ctypes.data for a in cls])
    assert g == grid, (g, grid)
    assert all(bool((a[g:] == -7).all()) for a in arrs) and all(bool((a[wgs * per_wg:] == -7).all()) for a in cls)
    tiles = list(zip(*[a[:tile_wgs].tolist() for a in arrs]))
    tail = list(zip(*[a[tile_wgs:g].tolist() for a in arrs]))
    items = [list(zip(cls[0][w * per_wg:(w + 1) * per_wg].tolist(), cls[1][w * per_wg:(w + 1) * per_wg].tolist())) for w in range(wgs)]
    return tiles, tail, items


def check_order(B, N, K, mode, keep):
    tiles, tail, items = order(B, N, K, mode, keep)
    tn_all = N // 256
    assert sorted((tm, tn) for tm, tn, _ in tiles) == [(m, n) for m in range(B) for n in range(tn_all)], "a tile twice or missing"
    assert all(dead == (0 if keep[tm] else 1) for tm, tn, dead in tiles), "a panel is dead exactly when its own image is dropped"
    deads = [dead for _, _, dead in tiles]
    D = sum(deads)
    assert deads == [1] * D + [0] * (len(tiles) - D), "dead tiles come first"
    per_chunk = [0] * 8
    for j in range(D, len(tiles)):
        per_chunk[(j - D) & 7] += 1
    assert max(per_chunk) - min(per_chunk) <= 1, "live tiles are not dealt evenly over the 8 chunks"
    # a chunk's live tiles are consecutive in the launch's live-tile order: chunk x = ranks [start_x, start_x + n_x)
    live_order = [(tm, tn) for g0 in range(0, B, 8) for tn in range(tn_all) for tm in range(g0, min(g0 + 8, B)) if keep[tm]]
    L, starts = len(live_order), []
    for x in range(8):
        starts.append(sum(per_chunk[:x]))
    for j in range(D, len(tiles)):
        i = j - D
        assert tiles[j][:2] == live_order[starts[i & 7] + (i >> 3)]
    assert L == len(tiles) - D
    # class-token workgroups: behind every tile, hold no tile, cover every (row tile, column tile) once
    assert all(t == (-1, -1, 0) for t in tail)
    flat = [it for w in items for it in w if it != (-1, -1)]
    assert sorted(flat) == [(r, c) for r in range(-(-B // 16)) for c in range(N // 16)], "a class-token item twice or missing"
    assert all(any(it != (-1, -1) for it in w) for w in items), "a class-token workgroup without work"


@pytest.mark.parametrize("N,K,mode", THREE)
def test_order_covers_every_tile_once_at_64_images(N, K, mode):
    rng = np.random.default_rng(257 + N)
    masks = [[1] * 64, [0] * 64, [1] + [0] * 63, [0] * 63 + [1], [b % 2 for b in range(64)]]
    masks += [(rng.random(64) < p).tolist() for p in (0.5, 0.5, 0.5, 0.3, 0.8)]
    with routed(image=0 if (N, K, mode) in KEPT else _lib.DENSE_IMAGE_ALWAYS):
        for keep in masks:
            check_order(64, N, K, mode, keep)
        assert order(64, N, K, mode, masks[0], drop=0.5)[0][:8] == order(64, N, K, mode, masks[0], drop=0.7)[0][:8]   # the hint moves no tile


@pytest.mark.parametrize("B", (1, 2, 5))
def test_every_mask_of_small_batches(B):
    with routed(image=_lib.DENSE_IMAGE_ALWAYS):
        for K in (640, 3840):
            for bits in itertools.product((0, 1), repeat=B):
                check_order(B, 512, K, 4, list(bits))
    with routed(image=_lib.DENSE_IMAGE_ALWAYS):
        check_order(13, 5120, 1280, 5, [b % 2 for b in range(13)])
        check_order(18, 3840, 1280, 0, [1] * 9 + [0] * 9)


def test_the_grid_depends_on_the_problem_and_the_hint_only():
    for N, K, mode in THREE:
        assert plan_image(64, N, K, mode, 0.5) == plan_image(64, N, K, mode, 0.5)
        assert plan_image(64, N, K, mode, 0.5)[:7] == plan_image(64, N, K, mode, 0.7)[:7]


def test_new_entry_points_are_declared_prototyped_exported_and_refuse_before_any_launch():
    L = _lib.lib()
    assert set(NEW) <= set(_lib.header_symbols()) and set(NEW) <= set(_lib._PROTOS)
    for name in NEW:
        assert hasattr(L, name)
    a, c = (list(_lib._PROTOS[n][1]) for n in ("octic_dense_gemm_nt_tokens_adaptive_cls", "octic_dense_gemm_nt_tokens_image"))
    assert c == a[:-1] + [ctypes.c_double, a[-1]]                    # drop in front of the stream
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20           # additions only
    out = (ctypes.c_int * 8)()
    assert L.octic_dense_gemm_plan_image(64 * TOK, 5120, 1280, 4, TOK, TOK, 1, 0.5, None) == -4
    assert L.octic_dense_gemm_plan_image(64 * TOK, 5120, 1280, 4, TOK, 0, 1, 0.5, out) == -1
    assert L.octic_dense_gemm_plan_image(64 * TOK, 5120, 1280, 4, TOK, 0, 0, 0.5, out) == 0     # no mask: rows_per_sample is not read
    sc = np.ones(64, dtype=np.float32)
    q = lambda N, s=sc.ctypes.data, cap=4096, drop=0.5: L.octic_dense_gemm_order_image(64 * TOK, N, 1280, 5, TOK, s, TOK, drop, cap, None,
                                                                                      None, None, 0, None, None)
    assert q(5120) == 1280 + 128 and q(1280) == -1 and q(5120, cap=1407) == -1 and q(5120, s=None) == -4 and q(5120, drop=0.0) == -1
    p, ss = 4096, 8192
    f = lambda M, s, rps, a=p: L.octic_dense_gemm_nt_tokens_image(a, p, M, 1280, 640, 640, 640, 0, p, None, 1280, None, None, None, 1,
                                                                  None, None, None, None, s, rps, p, TOK, 0, 0.5, None)
    assert f(771, ss, 0) == -1 and f(771, ss, 256) == -1 and f(771, ss + 2, 257) == -2 and f(771, ss, 257, a=None) == -4


def test_switch(monkeypatch):
    import octic_vits_amd.functional as OF
    from octic_vits_amd import ops
    monkeypatch.delenv("OCTIC_DENSE_IMAGE_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_DENSE_IMAGE_SKIP") is True       # on by default
    monkeypatch.setenv("OCTIC_DENSE_IMAGE_SKIP", "0")
    assert OF._skip_from_env("OCTIC_DENSE_IMAGE_SKIP") is False
    monkeypatch.setattr(OF, "DENSE_IMAGE_DROPPED", True)
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", True)
    assert ops._dense_image()
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", False)           # no mask reaches the launch: nothing to decide
    assert not ops._dense_image()
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", True)
    monkeypatch.setattr(OF, "DENSE_IMAGE_DROPPED", False)
    assert not ops._dense_image()
    assert ops.dense_plan_image(64 * TOK, 5120, 1280, 5, TOK, TOK, 0.5) == (True, 1408, 128, 10, 1280, 256, 132, True)
