"""CPU-only side of octic_dense_gemm_nt_tokens_adaptive (csrc/dense_gemm.hip dense_nt_adaptive_kernel): a masked one-round
launch of the 320-wide tile chooses its tile width on the device - 256 wide exactly while live panels * (N / 256) <= CUs.  The
rule and the eligibility come through octic_dense_gemm_plan_adaptive, what each workgroup gets through
octic_dense_gemm_order_adaptive (the kernel's own functions run on the host).

What the answers are compared with is built here or asked from the queries that were there before: the tiles of a width are
range(panels) x range(N // width), the forced-256 per-image launch is octic_dense_gemm_order_dropped under the tile knob, the
unmasked launch's order is the documented chunked deal over workgroup index & 7."""
import contextlib
import ctypes
import itertools

import numpy as np
import pytest

from octic_vits_amd import _lib

TOK = 257
CUS = 256        # what the plan assumes without a device (and what an MI355X has)
NEW = ("octic_dense_gemm_nt_tokens_adaptive", "octic_dense_gemm_plan_adaptive", "octic_dense_gemm_order_adaptive")


@contextlib.contextmanager
def routed(tile=0, image=0):
    try:
        _lib.route_override(_lib.ROUTE_DENSE_TILE, tile)
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, image)
        yield
    finally:
        _lib.route_override(_lib.ROUTE_DENSE_TILE, 0)
        _lib.route_override(_lib.ROUTE_DENSE_IMAGE, 0)


def plan_adaptive(B, N, K=128, mode=0, tokens=TOK, M=None, rps=TOK):
    out = (ctypes.c_int * 5)()
    assert _lib.lib().octic_dense_gemm_plan_adaptive(B * TOK if M is None else M, N, K, mode, tokens, rps, out) == 0
    return tuple(out)


def order_adaptive(B, N, K, keep, cap=4096):
    sc = np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(3)]
    width = ctypes.c_int(-7)
    g = _lib.lib().octic_dense_gemm_order_adaptive(B * TOK, N, K, 0, TOK, sc.ctypes.data, TOK, cap, *[a.ctypes.data for a in arrs],
                                                   ctypes.addressof(width))
    assert g > 0, g
    assert all(bool((a[g:] == -7).all()) for a in arrs)
    tm, tn, dead = [a[:g] for a in arrs]
    return tm.tolist(), tn.tolist(), dead.tolist(), width.value


def order_dropped(B, N, K, keep, cap=4096):
    sc = np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)
    arrs = [np.full(cap, -7, dtype=np.int32) for _ in range(5)]
    g = _lib.lib().octic_dense_gemm_order_dropped(B * TOK, N, K, 0, TOK, sc.ctypes.data, TOK, cap, *[a.ctypes.data for a in arrs])
    assert g > 0, g
    tm, tn, part, front, dead = [a[:g].tolist() for a in arrs]
    assert not any(part) and not any(front)
    return tm, tn, dead


def check_order(B, N, keep, tm, tn, dead, width):
    """The non-returning workgroups are every tile of `width` once, dead tiles first, the live ones dealt to workgroup index & 7
    in contiguous chunks whose sizes differ by at most one; returning workgroups only behind them."""
    tiles_n = N // width
    n = B * tiles_n
    assert all(t == -1 for t in tm[n:]) and all(t == -1 for t in tn[n:]) and not any(dead[n:]), "a workgroup past the tiles has work"
    got = list(zip(tm[:n], tn[:n]))
    assert sorted(got) == [(a, b) for a in range(B) for b in range(tiles_n)], "a tile twice or missing"
    for (a, _), d in zip(got, dead[:n]):
        assert bool(d) == (not keep[a])
    D = sum(dead[:n])
    assert all(dead[:D]) and not any(dead[D:n]), "the dead tiles do not sit together in front"
    counts = [sum(1 for bid in range(D, n) if bid & 7 == x) for x in range(8)]
    assert max(counts) - min(counts) <= 1
    return D


def test_rule_through_the_plan_query():
    """narrow iff live panels * (N / 256) <= CUs: 51 at N 1280 (5 x 51 = 255), 25 at N 2560 (10 x 25 = 250)."""
    eligible, grid, wide, narrow, max_live = plan_adaptive(64, 1280, 1280)
    assert (eligible, grid, wide, narrow, max_live) == (1, 320, 320, 256, 51)
    assert plan_adaptive(64, 2560, 1280)[4] == 25
    assert 5 * 51 <= CUS < 5 * 52 and 10 * 25 <= CUS < 10 * 26


def test_eligibility():
    assert plan_adaptive(64, 1280, 1280)[0] == 1
    assert plan_adaptive(64, 1280, 5120)[0] == 1                     # fc2 and its twin in the backward
    assert plan_adaptive(64, 640, 1280)[0] == 0                      # 256 does not divide N
    assert plan_adaptive(64, 640, 1280)[4] == -1
    assert plan_adaptive(64, 1280, 1280, mode=4)[0] == 0             # a fused tail
    assert plan_adaptive(64, 1280, 1280, tokens=0)[0] == 0           # classic panels
    assert plan_adaptive(70, 1280, 1280)[0] == 0                     # 280 tiles: a split front
    with routed(tile=5, image=1):
        assert plan_adaptive(1025, 1280, 128)[0] == 0                # more panels than the bitmap holds
        assert plan_adaptive(3, 1280, 128)[0:2] == (1, 15)
        assert plan_adaptive(52, 1280, 128)[0:2] == (1, 260)         # one round of 208 wide tiles; narrow only while <= 51 are live
    out = (ctypes.c_int * 5)()
    L = _lib.lib()
    assert L.octic_dense_gemm_plan_adaptive(64 * TOK, 1280, 1280, 0, TOK, 0, out) == -1
    assert L.octic_dense_gemm_plan_adaptive(64 * TOK, 1280, 1280, 0, TOK, 256, out) == -1
    assert L.octic_dense_gemm_plan_adaptive(64 * TOK, 1280, 1280, 0, TOK, TOK, None) == -4
    sc = np.ones(64, dtype=np.float32)
    q = lambda N, s=sc.ctypes.data, cap=4096: L.octic_dense_gemm_order_adaptive(64 * TOK, N, 1280, 0, TOK, s, TOK, cap, None, None,
                                                                               None, None)
    assert q(1280) == 320 and q(640) == -1 and q(1280, cap=319) == -1 and q(1280, s=None) == -4


@pytest.mark.parametrize("B", range(1, 11))
def test_every_mask_of_small_batches(B):
    """All 2^B masks at N 1280, K 128 (per-image panels and the 320-wide plan forced: the model would not choose them this
    small).  By the rule: narrow (5 B <= 256), a permutation of the tiles of the forced-256 per-image launch, dead first,
    per-XCD live counts within one tile.  Under 'always wide': octic_dense_gemm_order_dropped workgroup by workgroup, with
    returning workgroups behind it.  Under 'always narrow': what the rule gave."""
    N, K = 1280, 128
    for bits in itertools.product((0, 1), repeat=B):
        keep = list(bits)
        with routed(tile=4, image=1):
            ref_tm, ref_tn, ref_dead = order_dropped(B, N, K, keep)
        with routed(tile=5, image=1):
            assert plan_adaptive(B, N, K)[:2] == (1, 5 * B)
            tm, tn, dead, width = order_adaptive(B, N, K, keep)
            wide_tm, wide_tn, wide_dead = order_dropped(B, N, K, keep)
        assert width == 256
        assert sum(dead) == check_order(B, N, keep, tm, tn, dead, 256) == 5 * (B - sum(keep))
        assert sorted(zip(tm, tn)) == sorted(zip(ref_tm, ref_tn)) and len(ref_tm) == 5 * B
        assert (tm, tn, dead) == (ref_tm, ref_tn, ref_dead)          # (in fact the forced-256 launch's own order)
        with routed(tile=5 + _lib.DENSE_ADAPT_WIDE, image=1):
            tm, tn, dead, width = order_adaptive(B, N, K, keep)
        assert width == 320 and len(tm) == 5 * B and len(wide_tm) == 4 * B
        assert (tm[:4 * B], tn[:4 * B], dead[:4 * B]) == (wide_tm, wide_tn, wide_dead)
        check_order(B, N, keep, tm, tn, dead, 320)
        with routed(tile=5 + _lib.DENSE_ADAPT_NARROW, image=1):
            assert order_adaptive(B, N, K, keep) == (ref_tm, ref_tn, ref_dead, 256)


def test_seeded_masks_at_64_images():
    """2000 seeded masks at the headline shape: narrow exactly when at most 51 samples are kept; never a tile twice or missing at
    either width.  Keep probabilities cover both sides of the boundary."""
    B, N, K = 64, 1280, 1280
    rng = np.random.default_rng(1280 + 64)
    seen = {256: 0, 320: 0}
    at_boundary = set()
    for i in range(2000):
        p = (0.5, 0.74, 0.8, 0.9)[i % 4] if i % 8 else rng.random()
        keep = (rng.random(B) < p).tolist()
        if i % 16 == 1:                                               # exactly 51 / 52 kept, which random draws rarely give
            keep = [True] * (51 + (i // 16) % 2) + [False] * (13 - (i // 16) % 2)
            rng.shuffle(keep)
        tm, tn, dead, width = order_adaptive(B, N, K, keep)
        kept = sum(keep)
        assert width == (256 if kept <= 51 else 320), (kept, width)
        assert len(tm) == 320
        check_order(B, N, keep, tm, tn, dead, width)
        seen[width] += 1
        if kept in (51, 52):
            at_boundary.add(kept)
    assert seen[256] > 300 and seen[320] > 300 and at_boundary == {51, 52}


def test_edge_masks_at_64_images():
    """All kept: the wide choice, in the unmasked launch's own order (tile rank = chunk of workgroup & 7, tiles in groups of 8
    panels, column-major in a group), 64 returning workgroups behind.  All dropped: narrow (pinned: 0 x 5 <= 256), 320 dead tiles."""
    B, N, K = 64, 1280, 1280
    tm, tn, dead, width = order_adaptive(B, N, K, [1] * B)
    assert width == 320 and not any(dead)
    full = 256
    for bid in range(full):
        x, q8 = bid & 7, full >> 3
        tile = x * q8 + (bid >> 3)
        g, in_g = divmod(tile, 8 * 4)
        assert (tm[bid], tn[bid]) == (8 * g + in_g % 8, in_g // 8), bid
    assert tm[full:] == [-1] * 64 and tn[full:] == [-1] * 64
    tm, tn, dead, width = order_adaptive(B, N, K, [0] * B)
    assert width == 256 and all(dead) and len(dead) == 320
    check_order(B, N, [0] * B, tm, tn, dead, 256)


def test_new_entry_points_are_declared_prototyped_and_exported():
    L = _lib.lib()
    assert set(NEW) <= set(_lib.header_symbols()) and set(NEW) <= set(_lib._PROTOS)
    for name in NEW:
        assert hasattr(L, name)
    assert list(_lib._PROTOS["octic_dense_gemm_nt_tokens_adaptive"][1]) == list(_lib._PROTOS["octic_dense_gemm_nt_tokens_skip"][1])
    assert L.octic_abi_version() == _lib.ABI_VERSION                 # additions only


def test_launch_refusals_come_back_before_any_launch():
    L = _lib.lib()
    p, ss = 4096, 8192
    f = lambda M, s, rps, a=p: L.octic_dense_gemm_nt_tokens_adaptive(a, p, M, 1280, 128, 128, 128, 0, p, None, 1280, None, None, None,
                                                                     1, None, None, None, None, s, rps, p, TOK, None)
    assert f(771, ss, 0) == -1 and f(771, ss, 256) == -1 and f(771, ss + 2, 257) == -2 and f(771, ss, 257, a=None) == -4


def test_switch_is_read_from_the_environment_and_chooses_the_entry_point(monkeypatch):
    import octic_vits_amd.functional as OF
    from octic_vits_amd import ops
    monkeypatch.delenv("OCTIC_DENSE_NARROW", raising=False)
    assert OF._skip_from_env("OCTIC_DENSE_NARROW") is True    # on by default
    monkeypatch.setenv("OCTIC_DENSE_NARROW", "0")
    assert OF._skip_from_env("OCTIC_DENSE_NARROW") is False
    assert isinstance(OF.DENSE_NARROW_DROPPED, bool)
    monkeypatch.setattr(OF, "DENSE_NARROW_DROPPED", False)
    assert ops._dense_narrow() is False
    monkeypatch.setattr(OF, "DENSE_NARROW_DROPPED", True)
    assert ops._dense_narrow() is True
    # no mask, no choice: with DENSE_NT_SKIP_DROPPED off nothing reaches ops.dense_gemm_nt as sample_scale
    monkeypatch.setattr(OF, "DENSE_NT_SKIP_DROPPED", False)
    assert OF.dense_skip_scale(object(), TOK, 64 * TOK) is None
    assert ops.dense_plan_adaptive(64 * TOK, 1280, 1280, 0, TOK, TOK) == (True, 320, 320, 256, 51)
