"""CPU-only side of the dense NT GEMMs under a stochastic-depth mask (octic_dense_gemm_nt_tokens_skip): the kernel's own item
map asked through octic_dense_gemm_order_dropped (csrc/dense_gemm.hip dense_item_masked) - for every mask a permutation of the
unmasked launch's items, split-K front untouched, dead full tiles together in front, live full tiles in the unmasked tile order
dealt evenly over the XCDs -, the plan query, the switch, which factors travel to the kernel, and the refusals.

The unmasked launch's items are rebuilt here from the plan's grid and the documented schedule (tiles in groups of 8 row panels,
column-major inside a group; full tiles dealt in contiguous chunks to workgroup index & 7; the remaining tiles cut along K in
front of the grid), not from the function under test."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch

from octic_vits_amd import _lib

NEW = ("octic_dense_gemm_nt_tokens_skip", "octic_dense_gemm_plan_dropped", "octic_dense_gemm_order_dropped")
TOK = 257
CUS = 256        # what the plan assumes without a device (and what an MI355X has)


@contextlib.contextmanager
def routed(**knobs):
    ids = {"split": _lib.ROUTE_DENSE_SPLIT, "tile": _lib.ROUTE_DENSE_TILE, "image": _lib.ROUTE_DENSE_IMAGE}
    try:
        for k, v in knobs.items():
            _lib.route_override(ids[k], v)
        yield
    finally:
        for k in knobs:
            _lib.route_override(ids[k], 0)


def plan(M, N, K, mode, tokens):
    out = (ctypes.c_int * 4)()
    assert _lib.lib().octic_dense_gemm_plan(M, N, K, mode, tokens, out) == 0
    return tuple(out)


def order(M, N, K, mode, tokens, scale, rps, cap=4096):
    sc = np.ascontiguousarray(scale, dtype=np.float32)
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(5)]
    g = _lib.lib().octic_dense_gemm_order_dropped(M, N, K, mode, tokens, sc.ctypes.data, rps, cap, *[a.ctypes.data for a in arrs])
    assert g > 0, g
    assert all(bool((a[g:] == -7).all()) for a in arrs)
    return [a[:g] for a in arrs]          # tm, tn, part, in the split front, dead


def tile_panel(tile, tiles_m, tiles_n):
    per_group = 8 * tiles_n
    g = tile // per_group
    gsz = min(8, tiles_m - 8 * g)
    in_g = tile - g * per_group
    return 8 * g + in_g % gsz, in_g // gsz


def unmasked_items(M, N, K, mode, tokens, split):
    """[(tm, tn, part, front)] per workgroup of the unmasked launch; (-1, -1, 0, 0) = padding.  `split` = parts per front tile."""
    width, _, image, grid = plan(M, N, K, mode, tokens)
    tiles_m = M // tokens if image else -(-M // 256)
    tiles_n = -(-N // width)
    tiles = tiles_m * tiles_n
    full = tiles if grid == tiles else tiles // CUS * CUS
    rem = tiles - full
    tail_pad = grid - full
    assert tail_pad == (rem * split + 7) & ~7, (grid, tiles, full, split)
    items = []
    for bid in range(grid):
        if bid < tail_pad:
            if bid >= rem * split:
                items.append((-1, -1, 0, 0))
            else:
                items.append((*tile_panel(full + bid // split, tiles_m, tiles_n), bid % split, 1))
        else:
            j = bid - tail_pad
            x, q8, r8 = j & 7, full >> 3, full & 7
            tile = (x * (q8 + 1) if x < r8 else r8 * (q8 + 1) + (x - r8) * q8) + (j >> 3)
            items.append((*tile_panel(tile, tiles_m, tiles_n), 0, 0))
    return items, dict(tiles_m=tiles_m, tiles_n=tiles_n, full=full, rem=rem, tail_pad=tail_pad, image=image, grid=grid)


def panel_live(tm, M, rps, image, keep):
    m0 = tm * TOK + 1 if image else tm * 256
    m1 = min(m0 + 256, M)
    return m0 < M and any(keep[b] for b in range(m0 // rps, (m1 - 1) // rps + 1))


def check_mask(M, N, K, mode, tokens, rps, keep, base, info):
    """Every property of the item map for one mask; base / info = unmasked_items(...)."""
    tm, tn, part, front, dead = order(M, N, K, mode, tokens, [2.0 if k else 0.0 for k in keep], rps)
    got = list(zip(tm.tolist(), tn.tolist(), part.tolist(), front.tolist()))
    assert len(got) == info["grid"]
    assert sorted(got) == sorted(base), "not a permutation of the unmasked launch's items"
    tp = info["tail_pad"]
    assert got[:tp] == base[:tp], "the split-K front moved"
    live = [panel_live(t, M, rps, info["image"], keep) for t in range(info["tiles_m"])]
    for bid, (t, _, _, _) in enumerate(got):
        assert bool(dead[bid]) == (t >= 0 and not live[t]), (bid, t)
    d = dead[tp:]
    D = int(d.sum())
    assert bool(d[:D].all()) and not bool(d[D:].any()), "the dead full tiles do not sit together in front"
    # live full tiles: per workgroup index & 7 (the XCD) counts within one tile of each other, and each XCD walks a contiguous,
    # increasing range of the live tiles in the unmasked launch's tile order
    tile_no = {tile_panel(t, info["tiles_m"], info["tiles_n"]): t for t in range(info["full"])}
    live_order = sorted(tile_no[(a, b)] for a, b, _, _ in got[tp + D:])
    rank = {t: i for i, t in enumerate(live_order)}
    per_xcd = [[rank[tile_no[got[bid][:2]]] for bid in range(tp + D, info["grid"]) if bid & 7 == x] for x in range(8)]
    counts = [len(c) for c in per_xcd]
    assert max(counts) - min(counts) <= 1 <= info["tiles_n"], counts
    for c in per_xcd:
        assert c == list(range(c[0], c[0] + len(c))) if c else True, "an XCD's live tiles are not one contiguous chunk"
    return int(dead.sum())


SMALL = [
    # name, knobs, N, K, mode, split parts, ragged extra rows (classic only)
    ("classic", dict(image=2), 640, 256, 0, 1, 0),
    ("classic-wide", dict(image=2, tile=5), 640, 256, 0, 1, 0),
    ("classic-ragged", dict(image=2), 264, 128, 5, 1, 44),
    ("classic-split", dict(image=2, split=2), 264, 512, 4, 2, 0),
    ("classic-split-wide", dict(image=2, split=3, tile=5), 640, 1280, 0, 3, 0),
    ("image", dict(image=1), 640, 256, 0, 1, 0),
    ("image-narrow", dict(image=1, tile=4), 640, 256, 0, 1, 0),
    ("image-split", dict(image=1, split=2), 272, 512, 3, 2, 0),
]


@pytest.mark.parametrize("name,knobs,N,K,mode,split,extra", SMALL, ids=[s[0] for s in SMALL])
@pytest.mark.parametrize("B", range(1, 11))
def test_item_map_is_a_permutation_for_every_mask(B, name, knobs, N, K, mode, split, extra):
    """All 2^B masks (B <= 10) on classic and per-image panels, both tile widths, a forced split front, and a ragged last
    panel (M = 257 B + 44 with one factor per row: every image's rows carry its bit, the 44 extra rows the last image's)."""
    with routed(**knobs):
        tokens = TOK if not extra else 0
        M = B * TOK + extra
        base, info = unmasked_items(M, N, K, mode, tokens, split)
        assert info["image"] == name.startswith("image")
        assert (info["tail_pad"] > 0) == (split > 1)
        if "wide" in name or "narrow" in name:
            assert plan(M, N, K, mode, tokens)[0] == (320 if "wide" in name else 256)
        rps = TOK if not extra else 1
        seen_dead = 0
        for bits in itertools.product((0, 1), repeat=B):
            keep = list(bits) if not extra else [k for k in bits for _ in range(TOK)] + [bits[-1]] * extra
            seen_dead += check_mask(M, N, K, mode, tokens, rps, keep, base, info)
        assert seen_dead > 0
        # all kept: the unmasked launch's order, workgroup by workgroup
        tm, tn, part, front, dead = order(M, N, K, mode, tokens, [1.0] * (M // rps), rps)
        assert list(zip(tm.tolist(), tn.tolist(), part.tolist(), front.tolist())) == base and not dead.any()


BIG = [
    ("qkv-65-panels", 64, 3840, 1280, 0, 1, 2000),            # 975 full tiles, no front
    ("fc1-65-panels", 64, 5120, 1280, 4, 5, 300),             # 1280 full tiles + 20 tiles cut five ways in front
    ("dgrad-70-panels", 70, 1280, 1280, 0, None, 2000),       # per-image panels: the second bitmap word
    ("qkv-71-panels", 70, 3840, 1280, 0, None, 300),
]


@pytest.mark.parametrize("name,B,N,K,mode,split,count", BIG, ids=[b[0] for b in BIG])
def test_seeded_masks_at_the_headline_sizes(name, B, N, K, mode, split, count):
    with routed(**({"image": 1} if name == "dgrad-70-panels" else {})):
        _seeded(name, B, N, K, mode, split, count)


def _seeded(name, B, N, K, mode, split, count):
    M = B * TOK
    if split is None:      # parts per front tile, read off the all-kept order (the headline shapes' fronts are pinned above)
        _, _, part, front, _ = order(M, N, K, mode, TOK, [1.0] * B, TOK)
        split = int(part[front == 1].max()) + 1 if front.any() else 1
    base, info = unmasked_items(M, N, K, mode, TOK, split)
    assert info["tiles_m"] == {"qkv-65-panels": 65, "fc1-65-panels": 65, "dgrad-70-panels": 70, "qkv-71-panels": 71}[name]
    if name == "fc1-65-panels":
        assert (info["full"], info["rem"], info["tail_pad"]) == (1280, 20, 104)
    rng = np.random.default_rng(20 + B + N)
    dead_total = 0
    for i in range(count):
        keep = (rng.random(B) < (0.5 if i % 4 else rng.random())).tolist()
        dead_total += check_mask(M, N, K, mode, TOK, TOK, keep, base, info)
    assert dead_total > count


def test_masked_plan_is_the_unmasked_plan_and_refusals():
    L = _lib.lib()
    out, ref = (ctypes.c_int * 4)(), (ctypes.c_int * 4)()
    for (M, N, K, mode, tokens) in ((64 * TOK, 1280, 1280, 0, TOK), (64 * TOK, 5120, 1280, 4, TOK), (777, 264, 128, 5, 0),
                                    (64 * TOK, 1280, 5120, 0, TOK)):
        assert L.octic_dense_gemm_plan_dropped(M, N, K, mode, tokens, 1, out) == 0
        assert L.octic_dense_gemm_plan(M, N, K, mode, tokens, ref) == 0
        assert tuple(out) == tuple(ref)
    assert L.octic_dense_gemm_plan_dropped(771, 256, 128, 0, 0, 0, out) == -1
    assert L.octic_dense_gemm_plan_dropped(771, 256, 128, 0, 0, 256, out) == -1
    assert L.octic_dense_gemm_plan_dropped(771, 256, 128, 0, 0, 257, None) == -4
    sc = np.ones(4096, dtype=np.float32)
    q = lambda M, mode, rps, cap=64, s=sc.ctypes.data: L.octic_dense_gemm_order_dropped(M, 256, 128, mode, 0, s, rps, cap, None, None,
                                                                                      None, None, None)
    assert q(771, 0, 257) == 4
    assert q(771, 0, 0) == -1 and q(771, 0, 256) == -1 and q(771, 2, 257) == -1 and q(771, 0, 257, cap=3) == -1
    assert q(771, 0, 257, s=None) == -4
    assert q(1025 * 256, 0, 256, cap=4096) == -1                     # more panels than the bitmap holds: the unmasked kernel runs it


def test_launch_refusals_come_back_before_any_launch():
    L = _lib.lib()
    p, ss = 4096, 8192
    f = lambda M, s, rps, a=p, mode=0: L.octic_dense_gemm_nt_tokens_skip(a, p, M, 256, 128, 128, 128, mode, p, None, 256, None, None, None,
                                                                          1, None, None, None, None, s, rps, p, 0, None)
    assert f(771, ss, 0) == -1 and f(771, ss, -3) == -1              # a mask needs rows_per_sample > 0
    assert f(771, ss, 256) == -1                                     # ... that divides M
    assert f(771, ss + 2, 257) == -2                                 # sample_scale must be 4-byte aligned
    assert f(0, ss, 257) == -1
    assert f(771, ss, 257, a=None) == -4
    assert f(771, None, 0, a=p + 2) == -2                            # without a mask rows_per_sample is not looked at


def test_new_entry_points_are_declared_prototyped_and_exported():
    L = _lib.lib()
    assert set(NEW) <= set(_lib.header_symbols()) and set(NEW) <= set(_lib._PROTOS)
    for name in NEW:
        assert hasattr(L, name)
    args, base = _lib._PROTOS["octic_dense_gemm_nt_tokens_skip"][1], _lib._PROTOS["octic_dense_gemm_nt_tokens"][1]
    # the plain argument list with sample_scale, rows_per_sample in front of workspace, tokens, stream
    assert list(args) == list(base[:-3]) + [ctypes.c_void_p, ctypes.c_int] + list(base[-3:])
    assert L.octic_abi_version() == _lib.ABI_VERSION                 # additions only


def test_switch_is_read_from_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_DENSE_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_DENSE_SKIP") is True    # on by default
    monkeypatch.setenv("OCTIC_DENSE_SKIP", "0")
    assert OF._skip_from_env("OCTIC_DENSE_SKIP") is False
    monkeypatch.setenv("OCTIC_DENSE_SKIP", "1")
    assert OF._skip_from_env("OCTIC_DENSE_SKIP") is True
    assert isinstance(OF.DENSE_NT_SKIP_DROPPED, bool)


def test_only_per_sample_gpu_factors_reach_the_kernel(monkeypatch):
    """Exactly wgrad_skip_scale's conditions, under the dense switch."""
    import octic_vits_amd.functional as OF
    rs = torch.tensor([2.0, 0.0, 2.0])
    meta = torch.empty(3, device="meta")
    monkeypatch.setattr(type(meta), "is_cuda", property(lambda self: True), raising=False)
    cases = [(None, 17, 51, None), (rs, 17, 51, None), (meta, 17, 51, None), (meta, 17, 52, None), (meta, 1, 3, None),
             (meta, 17, 51, object()), (meta.double(), 17, 51, None)]
    monkeypatch.setattr(OF, "WGRAD_SKIP_DROPPED", True)
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", True)
    for r, rps, M, rows_to in cases:
        assert (OF.dense_skip_scale(r, rps, M, rows_to) is None) == (OF.wgrad_skip_scale(r, rps, M, rows_to) is None)
    assert OF.dense_skip_scale(meta, 17, 51) is not None
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", False)
    assert OF.dense_skip_scale(meta, 17, 51) is None and OF.wgrad_skip_scale(meta, 17, 51) is not None
