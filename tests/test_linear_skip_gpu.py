"""The octic MLP's row-local kernels with the stochastic-depth mask of their branch (include/octic_hip.h:
octic_linear_d8_fwd_skip, octic_gelu_d8_fwd_skip, octic_gelu_d8_bwd_skip).

The yardstick throughout is the UNMASKED launch of the same build, compared with torch.equal.

1. linear_d8_wreg_kernel<bf16, 0, SKIP>: rows of kept samples keep their bits for every kind of mask, at the full-k path
   (cin 160) and the guarded one (cin 32, 96), with samples of 257, 37, 8 and 1 rows (several samples per 32-row tile; but for
   8 x 40 no M is a multiple of 32, so the partial last tile is in play); a tile wholly inside dropped samples is NOT written (sentinel);
   a masked call with a fused tail is refused; a shape on the ring kernel computes every row.
2. D8-GELU forward and backward, bf16 (four channels per thread) and f32 (the generic kernels): input rows of dropped samples
   are NaN-poisoned and never read, their output rows are +0, every other row is the unmasked result.
3. One train.Trainer step of a small octic model with functional.LINEAR_SKIP_DROPPED on and off, eagerly and captured: same
   loss, same gradients, same parameters."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP = 2.0                       # 1 / keep at drop_path 0.5


def _masks(B):
    out = {"all kept": [KEEP] * B, "all dropped": [0.0] * B, "alternating": [KEEP * (b & 1) for b in range(B)],
           "first kept": [KEEP] + [0.0] * (B - 1), "last kept": [0.0] * (B - 1) + [KEEP]}
    for s in (1, 2):
        g = torch.Generator().manual_seed(200 + s)
        out[f"bernoulli {s}"] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).tolist()
    return out


def _row_keep(mask, rps):
    return (torch.tensor(mask, device=DEV) != 0).repeat_interleave(rps)


# ---- 1: the GEMM ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gemm_problem(cin, cout, M):
    """x, prepared weights, bias and the unmasked result (computed once per shape, never modified)."""
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(cin * 1000 + cout + M)
    x = torch.randn(M, 8 * cin, generator=g).to(torch.bfloat16).to(DEV)
    w32 = [(torch.randn(s, generator=g) * 0.1).to(DEV) for s in [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]]
    bias = torch.randn(cout, generator=g).to(DEV)
    wb, _ = ops.linear_prep(w32, None, cin, cout, torch.bfloat16, want_wb=True)
    ref = _gemm(x, wb, bias, cin, cout, None, 0)
    return x, wb, bias, ref


def _gemm(x, wb, bias, cin, cout, mask, rps, out=None):
    from octic_vits_amd import ops
    M = x.shape[0]
    y = out if out is not None else torch.full((M, 8 * cout), float("nan"), dtype=torch.bfloat16, device=DEV)
    ss = None if mask is None else torch.tensor(mask, dtype=torch.float32, device=DEV)
    ops.linear_fwd(ops.pview(x, cin), wb, bias, ops.pview(y, cout), M, cin, cout, torch.bfloat16, torch.bfloat16, x,
                   sample_scale=ss, skip_rps=rps)
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("rps,B", [(257, 7), (37, 20), (8, 40), (1, 100)])
@pytest.mark.parametrize("cin,cout", [(160, 640), (32, 64), (96, 96)])
def test_rows_of_kept_samples_keep_their_bits(cin, cout, rps, B):
    from octic_vits_amd import _lib
    M = rps * B                                      # (no multiple of 32 but 8 x 40: the partial last tile is in play)
    assert _lib.plan("octic_linear_d8_plan", M, cin, cout, _lib.BF16, _lib.BF16, 0)[0] == _lib.LINEAR_WREG
    x, wb, bias, ref = _gemm_problem(cin, cout, M)
    assert bool(torch.isfinite(ref.float()).all())
    for name, mask in _masks(B).items():
        y = _gemm(x, wb, bias, cin, cout, mask, rps)
        keep = _row_keep(mask, rps)
        assert torch.equal(y[keep], ref[keep]), (name, cin, cout, rps)


def test_tiles_inside_dropped_samples_are_not_written():
    """7 samples of 257 rows, samples 2 and 3 dropped: the 32-row tiles (16 tokens for the E pair rows) lying wholly inside rows
    514 .. 1027 keep the sentinel the output was filled with - the kernel skips, it does not merely agree."""
    cin, cout, rps, B = 160, 640, 257, 7
    x, wb, bias, ref = _gemm_problem(cin, cout, rps * B)
    mask = [KEEP, KEEP, 0.0, 0.0, KEEP, KEEP, KEEP]
    sentinel = torch.full((rps * B, 8 * cout), 0x7B7B, dtype=torch.int16, device=DEV)
    y = _gemm(x, wb, bias, cin, cout, mask, rps, out=sentinel.view(torch.bfloat16).clone())
    keep = _row_keep(mask, rps)
    assert torch.equal(y[keep], ref[keep])
    yi = y.view(torch.int16)
    lo, hi = 2 * rps, 4 * rps
    for tok_per_tile, cols in ((32, slice(0, 4 * cout)), (16, slice(4 * cout, 8 * cout))):
        t0, t1 = -(-lo // tok_per_tile), hi // tok_per_tile            # tiles [t0, t1) lie wholly inside the dropped rows
        assert t1 - t0 >= 14
        rows = slice(t0 * tok_per_tile, t1 * tok_per_tile)
        assert bool((yi[rows, cols] == 0x7B7B).all()), tok_per_tile


def test_a_masked_call_with_a_fused_tail_is_refused():
    from octic_vits_amd import ops
    cin, cout, rps, B = 32, 64, 37, 20
    x, wb, bias, _ = _gemm_problem(cin, cout, rps * B)
    y = torch.zeros(rps * B, 8 * cout, device=DEV)
    resid = torch.zeros_like(y)
    ss = torch.full((B,), KEEP, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ops.linear_fwd(ops.pview(x, cin), wb, bias, ops.pview(y, cout), rps * B, cin, cout, torch.bfloat16, torch.float32, x,
                       resid_v=ops.pview(resid, cout), sample_scale=ss, skip_rps=rps)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        ops.linear_fwd(ops.pview(x, cin), wb, bias, ops.pview(y, cout), rps * B, cin, cout, torch.bfloat16, torch.float32, x,
                       rs=ss, rps=rps, sample_scale=ss, skip_rps=rps)


def test_the_ring_kernel_computes_every_row():
    from octic_vits_amd import _lib
    cin, cout, rps, B = 640, 160, 37, 6
    M = rps * B
    assert _lib.plan("octic_linear_d8_plan", M, cin, cout, _lib.BF16, _lib.BF16, 0)[0] == _lib.LINEAR_RING
    x, wb, bias, ref = _gemm_problem(cin, cout, M)
    assert torch.equal(_gemm(x, wb, bias, cin, cout, [0.0, KEEP, 0.0, 0.0, KEEP, 0.0], rps), ref)


# ---- 2: the D8-GELU ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gelu_problem(c, M, dtype):
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(c + M)
    x = torch.randn(M, 8 * c, generator=g).to(dtype).to(DEV)
    dy = torch.randn(M, 8 * c, generator=g).to(dtype).to(DEV)
    y, gi = torch.empty_like(x), torch.empty_like(x)
    ops.gelu_fwd(ops.pview(x, c), ops.pview(y, c), M, c, dtype, x)
    ops.gelu_bwd(ops.pview(dy, c), ops.pview(x, c), ops.pview(gi, c), M, c, dtype, x)
    torch.cuda.synchronize()
    return x, dy, y, gi


def _is_plus_zero(t):
    return bool((t.view(torch.int16 if t.element_size() == 2 else torch.int32) == 0).all())


@pytest.mark.parametrize("rps,B", [(257, 3), (37, 5), (1, 50)])
@pytest.mark.parametrize("c", [640, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_gelu_reads_no_dropped_row_and_writes_zeros(dtype, c, rps, B):
    """bf16 runs gelu_fwd4 / gelu_bwd4, f32 the generic eight-channel kernels."""
    from octic_vits_amd import ops
    M = rps * B
    x, dy, y_ref, gi_ref = _gelu_problem(c, M, dtype)
    for name, mask in _masks(B).items():
        keep = _row_keep(mask, rps)
        xp, gp = x.clone(), dy.clone()
        xp[~keep] = float("nan")
        gp[~keep] = float("nan")
        ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
        y = torch.full_like(x, float("nan"))
        gi = torch.full_like(x, float("nan"))
        ops.gelu_fwd(ops.pview(xp, c), ops.pview(y, c), M, c, dtype, xp, sample_scale=ss, rows_per_sample=rps)
        ops.gelu_bwd(ops.pview(gp, c), ops.pview(xp, c), ops.pview(gi, c), M, c, dtype, xp, sample_scale=ss, rows_per_sample=rps)
        torch.cuda.synchronize()
        for got, ref in ((y, y_ref), (gi, gi_ref)):
            assert torch.equal(got[keep], ref[keep]), (name, c, rps)
            assert _is_plus_zero(got[~keep]), (name, c, rps)


# ---- 3: a training step -----------------------------------------------------------------------------------------------
def _model(img, embed, heads, depth, octic):
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(0)
    return OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                  img_size=img, patch_size=14, num_classes=10, embed_dim=embed, depth=depth, num_heads=heads,
                                  qkv_bias=True, init_scale=0.1, drop_path_rate=0.5, octic_equi_break_layer=octic).cuda()


@pytest.fixture
def injected_masks():
    """The same device-resident masks in every forward of a run (a captured step replays what it recorded): mask k of a forward
    is a fixed Bernoulli(0.5) draw scaled by 1 / keep."""
    import octic_vits_amd.d8_layers as L
    calls, cache = [0], {}
    for B in (4, 8):                                                 # made up front: nothing may be created while a step is captured
        for k in range(16):
            g = torch.Generator().manual_seed(500 + k)
            cache[(k, B)] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).to(DEV)

    def source(B, keep, device):
        k = calls[0] % 16
        calls[0] += 1
        return cache[(k, B)]

    L.drop_path_mask_source = source
    yield calls
    L.drop_path_mask_source = None


@pytest.fixture
def linear_switch():
    import octic_vits_amd.functional as OF
    before = OF.LINEAR_SKIP_DROPPED
    yield OF
    OF.LINEAR_SKIP_DROPPED = before


def _count_masked(monkeypatch):
    from octic_vits_amd import ops
    seen = {"linear": 0, "gelu": 0}
    lin, gf, gb = ops.linear_fwd, ops.gelu_fwd, ops.gelu_bwd

    def wrap(fn, key):
        def inner(*a, **k):
            seen[key] += k.get("sample_scale") is not None
            return fn(*a, **k)
        return inner

    monkeypatch.setattr(ops, "linear_fwd", wrap(lin, "linear"))
    monkeypatch.setattr(ops, "gelu_fwd", wrap(gf, "gelu"))
    monkeypatch.setattr(ops, "gelu_bwd", wrap(gb, "gelu"))
    return seen


def _step_both_ways(img, B, embed, heads, depth, octic, captured, calls, switch, seen, linear=2):
    from octic_vits_amd.train import Trainer, synthetic_batch
    x, y = synthetic_batch(B, 10, DEV, seed=3, img_size=img)
    results = []
    for on in (True, False):
        switch.LINEAR_SKIP_DROPPED = on
        calls[0] = 0
        seen.update(linear=0, gelu=0)
        tr = Trainer(_model(img, embed, heads, depth, octic), lr=1e-3)
        if captured:
            loss = tr.capture(x, y, warmup=1).replay(x, y).detach().clone()
        else:
            loss = tr.step(x, y).detach().clone()
            # per octic block: fc1's forward and fc2's input gradient (at T = 257 also qkv's forward and proj's input gradient);
            # the GELU forward and backward
            assert seen == ({"linear": linear * octic, "gelu": 2 * octic} if on else {"linear": 0, "gelu": 0}), seen
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


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_is_bitwise_with_and_without_skipping(captured, injected_masks, linear_switch, monkeypatch):
    """Two octic blocks and a standard one, 28 x 28 images at patch 14 (T = 5), embed_dim 256 (c = 32: fc1 and fc2's input
    gradient run the W-stationary kernel), 8 images, drop_path 0.5."""
    _step_both_ways(28, 8, 256, 4, 3, 2, captured, injected_masks, linear_switch, _count_masked(monkeypatch))


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_at_257_tokens(captured, injected_masks, linear_switch, monkeypatch):
    """224 x 224 (T = 257), 4 images, one octic block and a standard one at ViT-H's width (embed_dim 1280, 16 heads of 80:
    c = 160) - the shape at which the attention kernels skip, so qkv's forward and proj's input gradient get the mask too and
    all four short-K GEMMs run the W-stationary kernel."""
    from octic_vits_amd import ops
    assert ops.attn_skips_dropped(4, 257, 80, ld=(3840, 1280, 3840))
    _step_both_ways(224, 4, 1280, 16, 2, 1, captured, injected_masks, linear_switch, _count_masked(monkeypatch), linear=4)
