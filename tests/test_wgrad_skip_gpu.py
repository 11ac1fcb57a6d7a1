"""TN weight gradients that skip the token rows of samples a stochastic-depth mask drops (include/octic_hip.h:
octic_dense_wgrad_tn_skip / _tn_pair_skip; csrc/dense_wgrad.hip dense_tn_kernel<KW, true>).

sample_scale[b] == 0 promises that the dY rows of sample b are zero; the kernel then walks only the 64-row reduction steps that
touch a kept sample, inside the same row slabs.  The yardstick throughout is the UNMASKED launch of the same build on the same
operands (dY rows of dropped samples zeroed), compared with torch.equal: same slabs, same order of the f32 sums, same bits.
Results are written into NaN-filled tensors, so an element no workgroup wrote shows up.

1. one 256 x 256 tile, 8 samples of 257 rows (33 steps) at 1, 2, 3 and the automatic 16 row slabs (two steps each: many slabs
   without a live step), every kind of mask; 81 steps in one slab (the second 64-step word of the live-step bitmap);
2. the 320-wide tile (K = 320, 640); samples of 37 rows (a step spans three samples, the last step is partial) and of 1 row;
3. the pair launch; NaN in the X rows of skipped steps (they are not read); a two-block model step with the switch on and off,
   eagerly and captured."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
STEP = 64                     # token rows per reduction step (csrc/dense_wgrad.hip DW_BR)


def _route_slabs(n):
    from octic_vits_amd import _lib
    _lib.route_override(_lib.ROUTE_WGRAD_SLABS, n)


@functools.lru_cache(maxsize=None)
def _operands(M, N, K, integer=False):
    g = torch.Generator().manual_seed(M * 7 + N + 3 * K)
    if integer:
        dy = torch.randint(-2, 3, (M, N), generator=g).to(torch.bfloat16)
        x = torch.randint(-3, 4, (M, K), generator=g).to(torch.bfloat16)
    else:
        dy, x = torch.randn(M, N, generator=g).to(torch.bfloat16), torch.randn(M, K, generator=g).to(torch.bfloat16)
    return dy.to(DEV), x.to(DEV)


def _zeroed(dy, mask, rps):
    """dY as the backward pass leaves it: the rows of dropped samples are zero."""
    keep = (torch.tensor(mask, device=DEV) != 0).repeat_interleave(rps)
    return dy * keep[:, None].to(dy.dtype)


def _masks(B, seeds=(1, 2, 3)):
    """name -> per-sample factors (0 or 2 = 1 / keep at drop_path 0.5)."""
    out = {"all kept": [2.0] * B, "all dropped": [0.0] * B,
           "first kept": [2.0] + [0.0] * (B - 1), "last kept": [0.0] * (B - 1) + [2.0],
           "alternating": [2.0 * (b & 1) for b in range(B)],
           "first half dropped": [0.0] * (B // 2) + [2.0] * (B - B // 2),
           "second half dropped": [2.0] * (B // 2) + [0.0] * (B - B // 2)}
    for s in seeds:
        g = torch.Generator().manual_seed(100 + s)
        out[f"bernoulli {s}"] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * 2.0).tolist()
    return out


def _check(M, N, K, rps, slabs, masks):
    """Masked launch == unmasked launch on the same operands, for every mask, at `slabs` forced row slabs (0 = automatic)."""
    from octic_vits_amd import ops
    assert M % rps == 0
    dy, x = _operands(M, N, K)
    try:
        _route_slabs(slabs)
        for name, mask in masks.items():
            dyz = _zeroed(dy, mask, rps)
            want = ops.dense_wgrad_tn(dyz, x)
            ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
            got = ops.dense_wgrad_tn(dyz, x, out=torch.full((N, K), float("nan"), device=DEV), sample_scale=ss,
                                     rows_per_sample=rps)
            assert torch.equal(got, want), f"{name} (slabs {slabs}): {int((got != want).sum())} elements differ"
            if not any(mask):
                assert int(torch.count_nonzero(got)) == 0, name
            else:
                assert float(want.abs().max()) > 0
    finally:
        _route_slabs(0)


# ---- 1: one tile, 33 steps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slabs", [1, 2, 3, 0])
def test_tiny_wide_shape_every_mask(slabs):
    """N = K = 256, 8 samples of 257 rows.  Two slabs: 'first half dropped' leaves slab 0 (steps 0-15, samples 0-3) without a
    live step; automatic = 16 slabs of two steps, most of them empty under most masks."""
    if slabs == 0:
        from octic_vits_amd import _lib
        assert _lib.plan("octic_dense_wgrad_plan", 2056, 256, 0, 256, 256) == (256, 1, 16, 0)
    _check(8 * 257, 256, 256, 257, slabs, _masks(8))


def test_more_than_64_steps_in_a_slab():
    """20 samples of 257 rows in ONE slab: 81 steps, two words of the live-step bitmap; with samples 0-15 dropped the whole first
    word (steps 0-63, rows 0-4095) is dead."""
    masks = _masks(20, seeds=(1, 2))
    masks["first word dead"] = [0.0] * 16 + [2.0] * 4
    masks["second word dead"] = [2.0] * 15 + [0.0] * 5
    _check(20 * 257, 256, 256, 257, 1, masks)


# ---- 2: the 320-wide tile, short samples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [320, 640])
@pytest.mark.parametrize("slabs", [0, 2])
def test_320_wide_tile(K, slabs):
    from octic_vits_amd import _lib
    assert int(_lib.lib().octic_dense_wgrad_tile(2056, 256, K)) == 320
    _check(8 * 257, 256, K, 257, slabs, _masks(8))


@pytest.mark.parametrize("rps,B", [(37, 16), (1, 130)])
@pytest.mark.parametrize("slabs", [0, 1, 2])
def test_short_samples(rps, B, slabs):
    """37 rows per sample: M = 592 is 9 full steps and one of 16 rows (rows past M read as zero), a step spans three samples.
    One row per sample, 130 samples: a step is live if any of its 64 factors is non-zero."""
    masks = _masks(B)
    if rps == 1:
        masks["one live row per step"] = [2.0 if b in (5, 127, 129) else 0.0 for b in range(B)]
        masks["middle step dead"] = [0.0 if 64 <= b < 128 else 2.0 for b in range(B)]
    _check(B * rps, 256, 256, rps, slabs, masks)


# ---- 3: pair, unread rows, end to end ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("integer", [False, True])
def test_pair_launch_with_one_mask(integer):
    """octic_dense_wgrad_tn_pair_skip, N0 = 768, N1 = 256, K = 256: the masked pair equals the unmasked pair; with small-integer
    operands (every partial sum exact, as in test_dense_wgrad_pair_integer_exact_and_equal_to_two_launches) it also equals the two
    single masked launches whatever slab counts those pick."""
    from octic_vits_amd import ops
    B, rps, N0, N1, K = 8, 257, 768, 256, 256
    M = B * rps
    dy0, x0 = _operands(M, N0, K, integer)
    dy1, x1 = _operands(M, N1, K + 0, integer)
    x1 = x1.flip(0).contiguous()                                   # (a second activation, not x0 again)
    for name, mask in _masks(B).items():
        ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
        z0, z1 = _zeroed(dy0, mask, rps), _zeroed(dy1, mask, rps)
        w0, w1 = ops.dense_wgrad_tn_pair(z0, x0, z1, x1)
        nan = lambda n: torch.full((n, K), float("nan"), device=DEV)
        g0, g1 = ops.dense_wgrad_tn_pair(z0, x0, z1, x1, dw1=nan(N1), dw0=nan(N0), sample_scale=ss, rows_per_sample=rps)
        assert torch.equal(g0, w0) and torch.equal(g1, w1), name
        if integer:
            assert torch.equal(g0, ops.dense_wgrad_tn(z0, x0, sample_scale=ss, rows_per_sample=rps)), name
            assert torch.equal(g1, ops.dense_wgrad_tn(z1, x1, sample_scale=ss, rows_per_sample=rps)), name
            assert torch.equal(g0.double(), z0.double().t() @ x0.double()), name


@pytest.mark.parametrize("slabs", [1, 2, 0])
def test_skipped_steps_are_not_read(slabs):
    """NaN in the X rows of every step that lies wholly inside dropped samples: the masked result is the clean one."""
    from octic_vits_amd import ops
    B, rps, N, K = 8, 257, 256, 256
    M = B * rps
    dy, x = _operands(M, N, K)
    try:
        _route_slabs(slabs)
        for name, mask in _masks(B).items():
            dyz = _zeroed(dy, mask, rps)
            ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
            clean = ops.dense_wgrad_tn(dyz, x)
            xp, dead = x.clone(), 0
            for s in range(-(-M // STEP)):
                r0, r1 = s * STEP, min(s * STEP + STEP, M)
                if not any(mask[r0 // rps:(r1 - 1) // rps + 1]):
                    xp[r0:r1] = float("nan")
                    dead += 1
            assert dead > 0 or name == "all kept" or name.startswith("bernoulli")
            got = ops.dense_wgrad_tn(dyz, xp, sample_scale=ss, rows_per_sample=rps)
            assert torch.equal(got, clean), f"{name} (slabs {slabs}, {dead} poisoned steps)"
    finally:
        _route_slabs(0)


def _small_model():
    from functools import partial
    from octic_vits_amd.vit_models import vit_models
    torch.manual_seed(0)
    return vit_models(img_size=56, patch_size=14, embed_dim=256, depth=2, num_heads=4, num_classes=10, mlp_ratio=4,
                      qkv_bias=True, drop_path_rate=0.5, norm_layer=partial(torch.nn.LayerNorm, eps=1e-6)).to(DEV)


@pytest.fixture
def wgrad_switch():
    import octic_vits_amd.functional as OF
    before = OF.WGRAD_SKIP_DROPPED
    yield OF
    OF.WGRAD_SKIP_DROPPED = before


def _count_masked_launches(monkeypatch):
    from octic_vits_amd import ops
    seen = {"single": 0, "pair": 0}
    single, pair = ops.dense_wgrad_tn, ops.dense_wgrad_tn_pair

    def one(*a, **k):
        seen["single"] += k.get("sample_scale") is not None
        return single(*a, **k)

    def two(*a, **k):
        seen["pair"] += k.get("sample_scale") is not None
        return pair(*a, **k)

    monkeypatch.setattr(ops, "dense_wgrad_tn", one)
    monkeypatch.setattr(ops, "dense_wgrad_tn_pair", two)
    return seen


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_is_bitwise_with_and_without_skipping(captured, wgrad_switch, monkeypatch):
    """Two standard blocks (D = 256, 4 heads, MLP 1024, drop_path 0.5), 8 images of 17 tokens, bf16 autocast through
    train.Trainer (the paired qkv + proj launch and the batched finishes are on): one step with functional.WGRAD_SKIP_DROPPED on
    and off from the same seeds gives the same loss and the same .grad of every parameter - eagerly and as a captured step."""
    from octic_vits_amd.train import Trainer, synthetic_batch
    seen = _count_masked_launches(monkeypatch)
    x, y = synthetic_batch(8, 10, DEV, seed=3, img_size=56)
    results = []
    for on in (True, False):
        wgrad_switch.WGRAD_SKIP_DROPPED = on
        tr = Trainer(_small_model(), lr=1e-3)
        torch.manual_seed(11)                                       # the drop-path masks come from the device generator
        seen.update(single=0, pair=0)
        if captured:
            gs = tr.capture(x, y, warmup=1)
            loss = gs.replay(x, y).detach().clone()
        else:
            loss = tr.step(x, y).detach().clone()
            # per step and block: fc2 + fc1 on their own, qkv + proj as one launch
            assert seen == ({"single": 4, "pair": 2} if on else {"single": 0, "pair": 0}), seen
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
