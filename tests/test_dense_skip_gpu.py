"""csrc/dense_gemm.hip under a stochastic-depth mask (octic_dense_gemm_nt_tokens_skip): a live tile is computed by the code, K
range and plan of the unmasked launch, a dead tile stores +0 - so everything here is torch.equal / bit patterns, on random bf16
operands, against the unmasked launch of the same build.  No tolerance anywhere.

The schedule (classic / per-image panels, tile width, split-K front) is forced with the OCTIC_ROUTE_DENSE_* knobs and asserted
through the plan queries.  The masks are written out; panels_of() recomputes by the panel geometry which panels they kill and
every masked case asserts that it has a dead panel (and, on classic panels, a live panel that straddles a dropped sample), so
no case passes because nothing was skipped.  A forced split needs K >= 512 (a part keeps at least four K-tiles): the split
cases use K = 512 beside the K = 128 / 192 / 256 of the unsplit ones."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A5B
TOK = 257

# kept (1) / dropped (0) samples per batch size.  Classic panel tm = rows 256 tm .. 256 tm + 255 = the last tm rows of image
# tm - 1 and the first 256 - tm rows of image tm.
MASKS = {
    3: [1, 1, 0],                                   # panel 3 (rows 768-770 = image 2) dead; panel 2 straddles image 2
    5: [1, 0, 0, 1, 0],                             # panels 2 and 5 dead, 0 1 3 4 live (checked by hand in the test below)
    17: [1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1],
    70: [1 if b % 3 == 0 else 0 for b in range(70)],   # dead panels 2, 5, ..., 65, 68: both bitmap words
}


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


@contextlib.contextmanager
def routed(**knobs):
    L = lib()
    ids = {"split": L.ROUTE_DENSE_SPLIT, "tile": L.ROUTE_DENSE_TILE, "image": L.ROUTE_DENSE_IMAGE}
    try:
        for k, v in knobs.items():
            L.route_override(ids[k], v)
        yield
    finally:
        for k in knobs:
            L.route_override(ids[k], 0)


SCHEDULES = {"classic": dict(image=2), "image": dict(image=1), "split": dict(image=2, split=2),
             "classic256": dict(image=2, tile=4), "classic320": dict(image=2, tile=5),
             "image256": dict(image=1, tile=4), "image320": dict(image=1, tile=5), "split320": dict(image=2, split=2, tile=5)}


def check_plan(o, M, N, K, mode, tokens, schedule, rps):
    """The plan in force is the schedule the case is named after, and the masked plan is the unmasked one."""
    plan = o.dense_plan(M, N, K, mode, tokens)
    assert o.dense_plan_dropped(M, N, K, mode, tokens, rps) == plan
    tile, _, image, grid = plan
    assert image == schedule.startswith("image"), plan
    if schedule[-3:] in ("256", "320"):
        assert tile == int(schedule[-3:]), plan
    tiles = (M // TOK if image else -(-M // 256)) * -(-N // tile)
    if schedule.startswith("split"):
        assert K >= 512 and grid == (2 * tiles + 7) & ~7, plan         # every tile cut in two, in front
    else:
        assert grid == tiles, plan
    return plan


def panels_of(M, rps, image):
    """[(rows of the panel, samples its rows touch)] by the kernel's panel geometry."""
    out = []
    n = M // TOK if image else -(-M // 256)
    for tm in range(n):
        m0 = tm * TOK + 1 if image else tm * 256
        m1 = min(m0 + 256, M)
        out.append((range(m0, m1), sorted({m // rps for m in (m0, m1 - 1)} | set(range(m0 // rps, (m1 - 1) // rps + 1)))))
    return out


def row_classes(M, rps, image, keep):
    """(kept rows, rows that lie only in dead panels, dead panels, live panels that straddle a dropped sample) as index lists."""
    covered_live, covered_dead, dead, straddle = set(), set(), [], []
    for tm, (rows, samples) in enumerate(panels_of(M, rps, image)):
        if any(keep[s] for s in samples):
            covered_live.update(rows)
            if not all(keep[s] for s in samples):
                straddle.append(tm)
        else:
            covered_dead.update(rows)
            dead.append(tm)
    kept = [m for m in range(M) if keep[m // rps]]
    only_dead = sorted(covered_dead - covered_live)
    return kept, only_dead, dead, straddle


_OPERANDS = {}


def operands(M, N, K):
    """Random bf16 operands of one shape, shared by the cases of that shape and never modified."""
    key = (M, N, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 6:
            _OPERANDS.clear()
        g = torch.Generator(device=DEV).manual_seed(7919 * M + 31 * N + K)
        a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        b = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=DEV)
        h = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
        _OPERANDS[key] = (a, b, bias, h)
    return _OPERANDS[key]


def launch(o, a, b, bias, h, mode, tokens, ss=None, rps=0):
    """One launch -> tuple of its outputs (C, then C2 or the column sums where the mode has them)."""
    kw = dict(tokens=tokens, sample_scale=ss, rows_per_sample=rps)
    if mode in (3, 5):
        return tuple(o.dense_gemm_nt(a, b, mode, h=h, want_colsum=True, **kw))
    out = o.dense_gemm_nt(a, b, mode, bias=bias, **kw)
    return tuple(out) if isinstance(out, tuple) else (out,)


def scale_of(keep):
    return torch.tensor([2.0 if k else 0.0 for k in keep], dtype=torch.float32, device=DEV)


def is_plus_zero(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


def idx(rows):
    return torch.tensor(rows, dtype=torch.long, device=DEV)


# ---- the hand-checked mask ------------------------------------------------------------------------------------------------
def test_hand_checked_mask_geometry():
    kept, only_dead, dead, straddle = row_classes(5 * TOK, TOK, False, MASKS[5])
    assert dead == [2, 5] and straddle == [1, 3, 4]            # (panel 0 is image 0 alone: live, nothing dropped in it)
    assert only_dead == list(range(512, 768)) + list(range(1280, 1285))
    for B, keep in MASKS.items():
        assert len(keep) == B
        _, od, dead, straddle = row_classes(B * TOK, TOK, False, keep)
        assert dead and straddle and od
        assert row_classes(B * TOK, TOK, True, keep)[2] == [b for b in range(B) if not keep[b]]
    assert max(row_classes(70 * TOK, TOK, False, MASKS[70])[2]) >= 64                  # the second bitmap word


# ---- 1. kept rows and dead-panel rows ---------------------------------------------------------------------------------------
CASES = [(3, 256, 128, "classic"), (3, 320, 256, "image"), (5, 640, 256, "classic"), (5, 256, 128, "image"),
         (5, 256, 512, "split"), (17, 320, 256, "classic"), (17, 640, 128, "image"), (70, 256, 128, "classic"),
         (70, 320, 128, "image"), (70, 640, 192, "classic")]


@pytest.mark.parametrize("mode", (0, 1, 3, 4, 5, 6))
@pytest.mark.parametrize("B,N,K,schedule", CASES)
def test_kept_rows_are_the_unmasked_launch_and_dead_rows_are_zero(B, N, K, schedule, mode):
    o = ops()
    M, keep = B * TOK, MASKS[B]
    with routed(**SCHEDULES[schedule]):
        plan = check_plan(o, M, N, K, mode, TOK, schedule, TOK)
        a, b, bias, h = operands(M, N, K)
        kept, only_dead, dead, straddle = row_classes(M, TOK, plan[2], keep)
        assert dead and kept and only_dead and (plan[2] or straddle)
        want = launch(o, a, b, bias, h, mode, TOK)
        got = launch(o, a, b, bias, h, mode, TOK, scale_of(keep), TOK)
    outs = 2 if mode in (1, 4) else 1
    for i in range(outs):
        assert torch.equal(got[i][idx(kept)], want[i][idx(kept)]), f"output {i}: kept rows differ"
        assert is_plus_zero(got[i][idx(only_dead)]), f"output {i}: rows of dead panels are not +0"
        assert bool(torch.isfinite(got[i].float()).all())


@pytest.mark.parametrize("B,N,K,schedule", [(5, 320, 192, "classic256"), (5, 320, 192, "classic320"), (17, 640, 128, "image256"),
                                            (17, 640, 128, "image320"), (5, 640, 512, "split320"), (70, 320, 256, "classic320")])
def test_both_tile_widths_plain_mode(B, N, K, schedule):
    test_kept_rows_are_the_unmasked_launch_and_dead_rows_are_zero(B, N, K, schedule, 0)


# ---- 8. tile widths: every output element sees the same MFMA sequence over K at either width -------------------------------
@pytest.mark.parametrize("B,N,K", [(5, 320, 128), (5, 640, 256), (17, 320, 256), (17, 640, 128), (70, 320, 128)])
def test_masked_256_wide_tile_equals_the_unmasked_320_wide_tile_on_per_image_panels(B, N, K):
    """Plain mode on per-image panels, random bf16 operands: the masked launch on the 256-wide tile against the unmasked launch
    on the 320-wide tile - equal on every row of every kept sample, class-token rows included, +0 on the dead panels' rows; and
    the two unmasked launches are equal everywhere.  (What a narrower tile for masked N = 1280 launches would rest on.)"""
    o = ops()
    M, keep = B * TOK, MASKS[B]
    a, b, bias, h = operands(M, N, K)
    with routed(**SCHEDULES["image320"]):
        check_plan(o, M, N, K, 0, TOK, "image320", TOK)
        want = launch(o, a, b, bias, h, 0, TOK)[0]
    with routed(**SCHEDULES["image256"]):
        check_plan(o, M, N, K, 0, TOK, "image256", TOK)
        narrow = launch(o, a, b, bias, h, 0, TOK)[0]
        got = launch(o, a, b, bias, h, 0, TOK, scale_of(keep), TOK)[0]
    kept, only_dead, dead, _ = row_classes(M, TOK, True, keep)
    assert dead and any(m % TOK == 0 for m in kept)
    assert torch.equal(narrow, want), "the two tile widths differ without a mask"
    assert torch.equal(got[idx(kept)], want[idx(kept)]), "kept rows differ between the tile widths"
    assert is_plus_zero(got[idx(only_dead)])


# ---- 2. the backward contract: zero cotangent rows -> the same outputs AND column sums ----------------------------------------
@pytest.mark.parametrize("mode", (3, 5))
@pytest.mark.parametrize("B,N,K,schedule", [(5, 256, 192, "classic"), (5, 256, 512, "split"), (17, 320, 128, "image"),
                                            (70, 256, 128, "classic")])
def test_zero_rows_of_dropped_samples_give_the_unmasked_outputs_and_column_sums(B, N, K, schedule, mode):
    o = ops()
    M, keep = B * TOK, MASKS[B]
    with routed(**SCHEDULES[schedule]):
        check_plan(o, M, N, K, mode, TOK, schedule, TOK)
        a, b, bias, h = operands(M, N, K)
        rowkeep = scale_of(keep).ne(0).repeat_interleave(TOK)
        a0 = a * rowkeep[:, None].to(a.dtype)
        want = launch(o, a0, b, None, h, mode, TOK)
        got = launch(o, a0, b, None, h, mode, TOK, scale_of(keep), TOK)
    assert torch.equal(got[0], want[0])
    assert torch.equal(got[1], want[1]), "column sums differ"
    assert bool(want[1].abs().sum() > 0)


# ---- 4. edge masks -------------------------------------------------------------------------------------------------------
def other_shape_launch(o):
    q = torch.ones((130, 512), dtype=torch.bfloat16, device=DEV)
    o.dense_gemm_nt(q, q[:72], 0)


@pytest.mark.parametrize("mode", (0, 4, 5))
@pytest.mark.parametrize("B,N,K,schedule", [(5, 320, 256, "classic"), (5, 256, 512, "split"), (3, 640, 128, "image")])
def test_edge_masks(B, N, K, schedule, mode):
    """All kept = the unmasked launch everywhere.  All dropped = +0 everywhere the panels reach, column sums included, twice
    with another shape in between - and an all-kept launch afterwards still equals the unmasked one, so no ticket of the split
    front was left armed.  Exactly one kept."""
    o = ops()
    M = B * TOK
    with routed(**SCHEDULES[schedule]):
        plan = check_plan(o, M, N, K, mode, TOK, schedule, TOK)
        a, b, bias, h = operands(M, N, K)
        want = launch(o, a, b, bias, h, mode, TOK)
        for t, w in zip(launch(o, a, b, bias, h, mode, TOK, scale_of([1] * B), TOK), want):
            assert torch.equal(t, w), "all kept"
        patch = idx([m for m in range(M) if not plan[2] or m % TOK != 0])
        cls = idx([m for m in range(M) if plan[2] and m % TOK == 0])
        for _ in range(2):
            got = launch(o, a, b, bias, h, mode, TOK, scale_of([0] * B), TOK)
            for i in range(2 if mode == 4 else 1):
                assert is_plus_zero(got[i][patch]), "all dropped: a row is not +0"
                assert torch.equal(got[i][cls], want[i][cls])              # (per-image: the class-token launch computes its rows)
            if mode == 5 and not plan[2]:
                assert is_plus_zero(got[1]), "all dropped: column sums are not +0"
            elif mode == 5:                                              # (the class-token rows still add to them)
                assert bool(torch.isfinite(got[1]).all())
            other_shape_launch(o)
        for t, w in zip(launch(o, a, b, bias, h, mode, TOK, scale_of([1] * B), TOK), want):
            assert torch.equal(t, w), "all kept after all dropped"
        one = [0] * B
        one[B // 2] = 1
        kept, only_dead, dead, _ = row_classes(M, TOK, plan[2], one)
        got = launch(o, a, b, bias, h, mode, TOK, scale_of(one), TOK)
        assert dead and torch.equal(got[0][idx(kept)], want[0][idx(kept)]) and is_plus_zero(got[0][idx(only_dead)])


# ---- 5. sample sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 5))
@pytest.mark.parametrize("M,rps,keep", [
    (3 * TOK, TOK, MASKS[3]),
    # 21 samples of 37 rows: panel 0 = samples 0-6, panel 1 = samples 6-13, panel 2 = samples 13-20, panel 3 = sample 20 (rows 768-776)
    (777, 37, [1, 0, 1, 0, 0, 0, 0] + [0] * 6 + [0] * 7 + [0]),            # panels 1, 2, 3 dead; panel 0 spans seven samples
    (777, 37, [0] * 6 + [0] + [0] * 6 + [1] + [0] * 6 + [0]),              # sample 13 kept: panels 1 and 2 live, 0 and 3 dead
    (3 * TOK, 1, [0] * 256 + [0] * 255 + [1] + [0] * 256 + [0, 0, 0]),     # per-row factors: only row 511 kept -> panel 1 live
])
def test_sample_sizes(M, rps, keep, mode):
    o = ops()
    N, K = 256, 192
    assert len(keep) * rps == M
    with routed(image=2):
        check_plan(o, M, N, K, mode, 0, "classic", rps)
        a, b, bias, h = operands(M, N, K)
        kept, only_dead, dead, _ = row_classes(M, rps, False, keep)
        assert dead and kept and only_dead
        if rps == 37:
            assert max(len(s) for _, s in panels_of(M, rps, False)) > 2        # a panel spans more than two samples
        want = launch(o, a, b, bias, h, mode, 0)
        got = launch(o, a, b, bias, h, mode, 0, scale_of(keep), rps)
    assert torch.equal(got[0][idx(kept)], want[0][idx(kept)])
    assert is_plus_zero(got[0][idx(only_dead)])


# ---- 6. rows that only dead panels cover are not read ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 4, 5))
@pytest.mark.parametrize("B,N,K,schedule", [(5, 256, 192, "classic"), (5, 256, 512, "split"), (17, 320, 128, "image")])
def test_unread_rows_may_hold_nan(B, N, K, schedule, mode):
    o = ops()
    M, keep = B * TOK, MASKS[B]
    with routed(**SCHEDULES[schedule]):
        plan = check_plan(o, M, N, K, mode, TOK, schedule, TOK)
        a, b, bias, h = operands(M, N, K)
        kept, only_dead, dead, _ = row_classes(M, TOK, plan[2], keep)
        want = launch(o, a, b, bias, h, mode, TOK)
        ap, hp = a.clone(), h.clone()
        ap[idx(only_dead)] = float("nan")
        hp[idx(only_dead)] = float("nan")
        got = launch(o, ap, b, bias, hp, mode, TOK, scale_of(keep), TOK)
    for i in range(2 if mode == 4 else 1):
        assert torch.equal(got[i][idx(kept)], want[i][idx(kept)])
        assert is_plus_zero(got[i][idx(only_dead)])
    if mode == 5:
        assert bool(torch.isfinite(got[1]).all()), "a column sum saw a poisoned row"


# ---- 7. the dead tiles' zero stores stay inside [M, N] ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 4, 5))
@pytest.mark.parametrize("B,N,K,schedule", [(5, 264, 192, "classic"), (5, 264, 512, "split"), (3, 272, 128, "image")])
def test_zero_stores_honour_ldc_and_the_guards(B, N, K, schedule, mode):
    """Through the C ABI with ldc = N + 8 and outputs prefilled with a sentinel (N = 264 / 272: a last column tile of 8 / 16)."""
    o, L = ops(), lib()
    M, keep = B * TOK, MASKS[B]
    with routed(**SCHEDULES[schedule]):
        plan = check_plan(o, M, N, K, mode, TOK, schedule, TOK)
        a, b, bias, h = operands(M, N, K)
        kept, only_dead, dead, _ = row_classes(M, TOK, plan[2], keep)
        want = launch(o, a, b, bias if mode != 5 else None, h, mode, TOK)
        ws = o._dense_ws(M, N, K, a.device)
        guarded = lambda: torch.full((M + 8, N + 8), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        c, c2, hg = guarded(), guarded(), guarded()
        hg[:M, :N] = h
        cs = torch.full((plan[1] + 4, N), float("nan"), device=DEV)
        P = o._p
        L.check(L.lib().octic_dense_gemm_nt_tokens_skip(
            P(a), P(b), M, N, K, K, K, mode, P(c), P(c2) if mode == 4 else None, N + 8, P(bias) if mode != 5 else None, None, None,
            1, None, None, P(hg) if mode == 5 else None, P(cs) if mode == 5 else None, P(scale_of(keep)), TOK, P(ws), TOK,
            o._stream(a)))
        torch.cuda.synchronize()
    for t in (c, c2, hg):
        bits = t.view(torch.int16)
        assert bool((bits[M:] == SENTINEL).all()) and bool((bits[:M, N:] == SENTINEL).all()), "a guard cell was written"
    outs = [c, c2] if mode == 4 else [c]
    for i, t in enumerate(outs):
        assert torch.equal(t[:M, :N][idx(kept)], want[i][idx(kept)])
        assert is_plus_zero(t[:M, :N][idx(only_dead)])
    if mode != 4:
        assert bool((c2.view(torch.int16) == SENTINEL).all())
    if mode == 5:
        assert bool(cs[plan[1]:].isnan().all()) and not bool(cs[:plan[1]].isnan().any())
        dead_rows = idx([2 * tm + w for tm in dead for w in (0, 1)])
        assert is_plus_zero(cs[dead_rows]), "the column-sum slab rows of a dead panel are not +0"
    else:
        assert bool(cs.isnan().all())


def test_masks_the_kernel_does_not_take_and_refusals():
    """Mode 2 through the C ABI ignores the mask (it computes every row); a bad rows_per_sample is OCTIC_ESHAPE."""
    o, L = ops(), lib()
    M, N, K = 3 * TOK, 256, 128
    a, b, bias, h = operands(M, N, K)
    ss = scale_of(MASKS[3])
    with pytest.raises(ValueError):
        o.dense_gemm_nt(a, b, 2, x=torch.zeros(M, N, device=DEV), sample_scale=ss, rows_per_sample=TOK)
    c = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    P = o._p
    call = lambda mode, rps, x=None, out=None: L.lib().octic_dense_gemm_nt_tokens_skip(
        P(a), P(b), M, N, K, K, K, mode, P(c), None, N, None, None, None, 1, P(x), P(out), None, None, P(ss), rps,
        P(o._dense_ws(M, N, K, a.device)), 0, o._stream(a))
    assert call(0, 0) == -1 and call(0, -3) == -1 and call(0, 100) == -1
    x = torch.zeros(M, N, device=DEV)
    out = torch.empty_like(x)
    assert call(2, TOK, x, out) == 0
    assert torch.equal(c, o.dense_gemm_nt(a, b, 0))                          # every row computed


# ---- 9. the trainer ---------------------------------------------------------------------------------------------------------
def _small_model():
    from functools import partial
    from octic_vits_amd.vit_models import vit_models
    torch.manual_seed(0)
    return vit_models(img_size=224, patch_size=14, embed_dim=256, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                      qkv_bias=True, drop_path_rate=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).to(DEV)


@pytest.fixture
def dense_switch():
    import octic_vits_amd.functional as OF
    before = OF.DENSE_NT_SKIP_DROPPED
    yield OF
    OF.DENSE_NT_SKIP_DROPPED = before


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_is_bitwise_with_and_without_skipping(captured, dense_switch, monkeypatch):
    """Two standard blocks (D = 256, 4 heads, MLP 1024, drop_path 0.5), 16 images of 257 tokens (17 classic panels), bf16
    autocast through train.Trainer: one step with functional.DENSE_NT_SKIP_DROPPED on and off from the same seeds gives the same
    loss, the same .grad and the same parameters - eagerly and as a captured step.  The eager run also counts the masked
    launches (eight per block) and checks from the masks they carried that at least one launch had a dead panel."""
    from octic_vits_amd import ops as o
    from octic_vits_amd.train import Trainer, synthetic_batch
    seen = []
    real = o.dense_gemm_nt

    def spy(a, *args, **kw):
        ss = kw.get("sample_scale")
        if ss is not None and not captured:
            seen.append((a.shape[0], kw["rows_per_sample"], ss.detach().cpu().tolist()))
        elif ss is not None:
            seen.append(None)
        return real(a, *args, **kw)

    monkeypatch.setattr(o, "dense_gemm_nt", spy)
    x, y = synthetic_batch(16, 10, DEV, seed=3, img_size=224)
    results = []
    for on in (True, False):
        dense_switch.DENSE_NT_SKIP_DROPPED = on
        tr = Trainer(_small_model(), lr=1e-3)
        torch.manual_seed(11)
        del seen[:]
        if captured:
            gs = tr.capture(x, y, warmup=1)
            loss = gs.replay(x, y).detach().clone()
            assert bool(seen) == on
        else:
            loss = tr.step(x, y).detach().clone()
            assert len(seen) == (16 if on else 0), len(seen)
            if on:
                assert all(rps == TOK and M == 16 * TOK for M, rps, _ in seen)
                assert any(row_classes(M, rps, False, [v != 0 for v in ss])[2] for M, rps, ss in seen), "no launch had a dead panel"
        torch.cuda.synchronize()
        results.append((loss, {n: p.grad.detach().clone() for n, p in tr.raw_model.named_parameters() if p.grad is not None},
                        [p.detach().clone() for p in tr.raw_model.parameters()]))
    (la, ga, pa), (lb, gb, pb) = results
    assert torch.equal(la, lb) and bool(torch.isfinite(la).all())
    assert set(ga) == set(gb) and len(ga) > 20
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
