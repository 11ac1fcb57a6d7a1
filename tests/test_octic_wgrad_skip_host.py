"""CPU-only side of the octic weight gradient under a stochastic-depth mask (octic_linear_d8_wgrad_skip): the steps every
(irrep group, row split) of a masked wgrad_ring_kernel launch walks, asked from octic_linear_d8_wgrad_order_dropped - the host
query that runs the kernel's own liveness and share rules (csrc/wgrad.hip: wg_step_live, wg_share_begin).

A step is 32 LDS rows of a group from its row 0; row mm of the pair group (E, group 0 of the launch, 2 M rows) is token
mm >> 1.  The liveness the tests expect is computed here, independently, from the token rows a step covers."""
import ctypes
import random

import pytest

from octic_vits_amd import _lib

BF16, F32 = _lib.BF16, _lib.F32
KEEP = 2.0
CIN, COUT = 160, 160


def _order(M, cin, cout, splits, mask, rps, dtype=BF16, cap=None):
    L = _lib.lib()
    cap = 5 * (2 * M // 32 + 2) if cap is None else cap
    ss = (ctypes.c_float * len(mask))(*mask)
    og, osp, ot = ((ctypes.c_int * max(cap, 1))() for _ in range(3))
    n = L.octic_linear_d8_wgrad_order_dropped(M, cin, cout, dtype, splits, ss, rps, cap, og, osp, ot)
    if n < 0:
        return n
    return [(og[i], osp[i], ot[i]) for i in range(n)]


def _live_steps(M, mask, rps, pair):
    """Independent of the library: step t covers LDS rows [32 t, 32 t + 32) clipped to the group's rows; pair rows map to
    tokens by >> 1; live = some covered token row lies in a sample with a non-zero factor."""
    rows = 2 * M if pair else M
    out = []
    for t in range((rows + 31) // 32):
        toks = {(mm >> 1) if pair else mm for mm in range(32 * t, min(32 * t + 32, rows))}
        if any(mask[tok // rps] != 0 for tok in toks):
            out.append(t)
    return out


def _masks(B):
    out = {"all kept": [KEEP] * B, "none kept": [0.0] * B, "one kept": [0.0] * (B - 1) + [KEEP],
           "alternating": [KEEP * (b & 1) for b in range(B)]}
    for s in (1, 2):
        r = random.Random(300 + s)
        out[f"random {s}"] = [KEEP * (r.random() < 0.5) for _ in range(B)]
    return out


def _plan_splits(M, cin, cout):
    return _lib.plan("octic_linear_d8_wgrad_plan", M, cin, cout, BF16)[2]


def _check(M, cin, cout, splits, mask, rps):
    got = _order(M, cin, cout, splits, mask, rps)
    assert not isinstance(got, int), got
    assert got == sorted(got)                                        # groups, splits and a split's steps ascend
    for g in range(5):
        pair = g == 0
        S = splits if pair else (splits + 1) // 2
        live = _live_steps(M, mask, rps, pair)
        walked = [t for gg, _, t in got if gg == g]
        assert walked == live                                        # every live step exactly once, no dead step
        shares = [sum(1 for gg, s, _ in got if gg == g and s == sp) for sp in range(S)]
        assert sum(shares) == len(live) and max(shares) - min(shares) <= 1
        assert all(0 <= s < S for gg, s, _ in got if gg == g)
        # split s takes the ranks [L s / S, L (s + 1) / S)
        L_ = len(live)
        assert shares == [L_ * (sp + 1) // S - L_ * sp // S for sp in range(S)]
    return got


@pytest.mark.parametrize("rps", [5, 33, 257])
@pytest.mark.parametrize("B", [4, 6, 64])
def test_every_live_step_is_walked_once_in_even_shares(rps, B):
    M = rps * B
    assert _lib.plan("octic_linear_d8_wgrad_plan", M, CIN, COUT, BF16)[0] == _lib.WGRAD_RING
    for splits in sorted({1, 2, _plan_splits(M, CIN, COUT)}):
        for name, mask in _masks(B).items():
            got = _check(M, CIN, COUT, splits, mask, rps)
            if name == "none kept":
                assert got == []


def test_fewer_live_steps_than_splits_leave_empty_shares():
    """One kept sample of 5 rows among 64: the one-dimensional groups have 1 or 2 live steps, E 1 or 2, under the plan's splits."""
    rps, B = 5, 64
    M = rps * B
    splits = _plan_splits(M, CIN, COUT)
    assert splits >= 2
    mask = [0.0] * B
    mask[10] = KEEP                                                  # tokens 50 .. 54: step 1 of A1, step 3 of E (rows 100 .. 109)
    got = _check(M, CIN, COUT, splits, mask, rps)
    assert [(g, t) for g, _, t in got] == [(0, 3), (1, 1), (2, 1), (3, 1), (4, 1)]
    for g, s, _ in got:                                              # L = 1: the last split takes it (ranks [s / S, (s + 1) / S))
        assert s == (splits if g == 0 else (splits + 1) // 2) - 1


def test_a_step_that_straddles_a_kept_and_a_dropped_sample_is_live():
    rps, B = 33, 4
    M = rps * B                                                      # 132 tokens: steps of 32 tokens (16 for E)
    mask = [0.0, KEEP, 0.0, 0.0]                                     # tokens 33 .. 65
    got = _check(M, CIN, COUT, 1, mask, rps)
    assert [t for g, _, t in got if g == 1] == [1, 2]                # tokens 32 .. 63 (one dropped row, 31 kept) and 64 .. 95
    assert [t for g, _, t in got if g == 0] == [2, 3, 4]             # E rows 64 .. 159 = tokens 32 .. 79: token = row >> 1
    # the neighbours that only touch dropped samples are dead
    assert 0 not in [t for g, _, t in got if g == 1] and 5 not in [t for g, _, t in got if g == 0]


def test_pair_rows_map_to_tokens_by_a_shift():
    rps, B = 5, 6
    M = rps * B                                                      # 30 tokens, E has 60 rows: steps 0 (tokens 0 .. 15), 1 (16 .. 29)
    for b in range(B):
        mask = [0.0] * B
        mask[b] = KEEP
        got = _order(M, CIN, COUT, 1, mask, rps)
        toks = range(rps * b, rps * b + rps)
        assert [t for g, _, t in got if g == 0] == sorted({tok // 16 for tok in toks})
        assert [t for g, _, t in got if g == 1] == [0]


def test_vit_h_shares_are_the_even_deal():
    """ViT-H at batch 64 (M = 64 x 257), drop_path 0.5: every split of every launch walks at most 0.55 of the steps a fixed
    split holds, for seeded half-kept masks (the fullest fixed split of an in-place skip is 0.83 - 1.00 live)."""
    rps, B = 257, 64
    M = rps * B
    seen = set()
    for cin, cout in ((160, 480), (160, 160), (160, 640), (640, 160)):
        splits = _plan_splits(M, cin, cout)
        seen.add(splits)
        for seed in range(3):
            r = random.Random(900 + seed)
            kept = set(r.sample(range(B), B // 2))
            mask = [KEEP if b in kept else 0.0 for b in range(B)]
            got = _check(M, cin, cout, splits, mask, rps)
            for g in range(5):
                S = splits if g == 0 else (splits + 1) // 2
                T = ((2 * M if g == 0 else M) + 31) // 32
                worst = max(sum(1 for gg, s, _ in got if gg == g and s == sp) for sp in range(S))
                assert worst <= 0.55 * (T / S) + 1, (cin, cout, g, worst, T, S)
    assert seen == {21, 28, 32}


def test_unmasked_launches_and_bad_masks_are_refused():
    L = _lib.lib()
    mask = [KEEP, 0.0, KEEP, 0.0]
    assert _order(4 * 33, CIN, COUT, 2, mask, 33, dtype=F32) == -1             # f32: the tiled kernel
    assert _order(4 * 33, 96, 96, 2, mask, 33) == -1                           # a 96-wide shape: the tiled kernel
    assert _order(4 * 33, CIN, COUT, 2, mask, 32) == -1                        # M % rows_per_sample
    assert _order(4 * 33, CIN, COUT, 2, mask, 0) == -1
    assert _order(4 * 33, CIN, COUT, 2, mask, 33, cap=3) == -1                 # cap too small
    big = 65568                                                                # E: 131136 rows = 4098 steps > 4096
    assert _order(big, CIN, COUT, 2, [KEEP] * (big // 32), 32) == -1
    assert isinstance(_order(65536, CIN, COUT, 2, [KEEP] * 2048, 32), list)    # 4096 steps: masked
    ss = (ctypes.c_float * 4)(*mask)
    o = (ctypes.c_int * 64)()
    assert L.octic_linear_d8_wgrad_order_dropped(132, CIN, COUT, BF16, 2, None, 33, 64, o, o, o) == -4
    assert L.octic_linear_d8_wgrad_order_dropped(132, CIN, COUT, BF16, 2, ss, 33, 64, None, o, o) == -4


def test_entry_point_is_declared_and_rejects_before_any_launch():
    L = _lib.lib()
    names = ["octic_linear_d8_wgrad_skip", "octic_linear_d8_wgrad_order_dropped"]
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._PROTOS)
    args, base = _lib._PROTOS["octic_linear_d8_wgrad_skip"][1], _lib._PROTOS["octic_linear_d8_wgrad"][1]
    assert list(args) == list(base[:-1]) + [ctypes.c_void_p, ctypes.c_int] + list(base[-1:])
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20                      # additions only
    v = _lib.OcticView()
    for i in range(5):
        v.ptr[i], v.ld[i] = 4096 + 64 * i, 8 * 160
    p, ss = 4096, 8192
    f = lambda M, s, rps: L.octic_linear_d8_wgrad_skip(ctypes.byref(v), ctypes.byref(v), M, 160, 160, BF16, p, 2, s, rps, None)
    assert f(132, ss, 0) == -1 and f(132, ss, -3) == -1 and f(132, ss, 32) == -1
    assert f(132, ss + 2, 33) == -2
    assert f(0, ss, 33) == -1


def test_switch_and_mask_rules(monkeypatch):
    import torch
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_LINEAR_WGRAD_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_LINEAR_WGRAD_SKIP") is True
    monkeypatch.setenv("OCTIC_LINEAR_WGRAD_SKIP", "0")
    assert OF._skip_from_env("OCTIC_LINEAR_WGRAD_SKIP") is False
    assert isinstance(OF.LINEAR_WGRAD_SKIP_DROPPED, bool)
    monkeypatch.setattr(OF, "LINEAR_WGRAD_SKIP_DROPPED", True)
    assert OF.linear_wgrad_skip_scale(torch.zeros(3), 17, 51) is None           # a CPU tensor: no kernel reads it
    meta = torch.empty(3, device="meta")                                        # passes for a GPU tensor as far as the shape rules go
    monkeypatch.setattr(type(meta), "is_cuda", property(lambda self: True), raising=False)
    # the mask asks no other switch
    for name in ("LINEAR_SKIP_DROPPED", "RING_SKIP_DROPPED", "ATTN_SKIP_DROPPED", "ROW_SKIP_DROPPED", "WGRAD_SKIP_DROPPED",
                 "DENSE_NT_SKIP_DROPPED"):
        for on in (True, False):
            monkeypatch.setattr(OF, name, on)
            assert OF.linear_wgrad_skip_scale(meta, 17, 51) is not None
    assert OF.linear_wgrad_skip_scale(None, 17, 51) is None                     # eval, drop_path 0
    assert OF.linear_wgrad_skip_scale(meta, 17, 52) is None                     # rps * B != M
    assert OF.linear_wgrad_skip_scale(meta, 1, 3) is None                       # one factor per row: ragged
    assert OF.linear_wgrad_skip_scale(meta.double(), 17, 51) is None
    monkeypatch.setattr(OF, "LINEAR_WGRAD_SKIP_DROPPED", False)
    assert OF.linear_wgrad_skip_scale(meta, 17, 51) is None
