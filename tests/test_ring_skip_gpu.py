"""The ring kernel with the stochastic-depth mask of its branch (include/octic_hip.h: octic_linear_d8_fwd_dropped;
csrc/gemm.hip linear_d8_ring_kernel<.., SKIP>).

The yardstick throughout is the UNMASKED launch of the same build, compared with torch.equal.  Every output is pre-filled with
NaN, so an item that no workgroup ran shows.  A tile is 128 GEMM rows: 128 tokens of a one-dimensional irrep (columns
[0, 4c) of a packed row), 64 tokens of the E irrep (columns [4c, 8c)); it is dead when all its tokens belong to dropped samples.

1. Plain launch (the input gradients of fc1 and qkv): x rows of dropped samples are zero, as the contract says - except that
   the rows of wholly dead tiles are NaN, which a kernel that read them would carry into the result.  Result == the unmasked
   launch on the zeroed x, finite, and the bit pattern of +0 in dead tiles.
2. Fused launch (fc2 + residual: bias, column scale, rs = the mask, f32 residual stream): x random, NaN in dead tiles.
   Result == the unmasked launch on the clean x; dead tiles hold the residual's bits.
   Both at the wide tile (cin 640, cout 160: NT = 10, S = 2) and the narrow one (cin 192, cout 96: NT = 5, S = 3), samples of
   257, 37, 64 (E tiles aligned to samples) and 1 rows, and a launch of fewer than 128 rows.
3. A shape on the W-stationary kernel ignores the mask: every row computed.
4. One train.Trainer step of a small octic model whose fc2 and input gradients run the ring kernel, with
   functional.RING_SKIP_DROPPED on and off, eagerly and captured: same loss, gradients and parameters."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP = 2.0                       # 1 / keep at drop_path 0.5
SHAPES = [(640, 160, 160), (192, 96, 80)]                              # cin, cout, columns per ring tile
SAMPLES = [(257, 7), (37, 20), (64, 9), (1, 300), (37, 3)]             # rows per sample, samples (the last: M = 111 < 128)


def _masks(B):
    out = {"all kept": [KEEP] * B, "all dropped": [0.0] * B, "alternating": [KEEP * (b & 1) for b in range(B)],
           "one kept": [0.0] * (B // 2) + [KEEP] + [0.0] * (B - B // 2 - 1),
           "one dropped": [KEEP] * (B // 2) + [0.0] + [KEEP] * (B - B // 2 - 1)}
    for s in (1, 2):
        g = torch.Generator().manual_seed(300 + s)
        out[f"bernoulli {s}"] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).tolist()
    return out


def _dead_rows(mask, rps, tokens_per_tile):
    """bool [M]: the token rows of tiles that cover dropped samples only."""
    dropped = (torch.tensor(mask) == 0).repeat_interleave(rps)
    M = dropped.numel()
    dead = torch.zeros(M, dtype=torch.bool)
    for t0 in range(0, M, tokens_per_tile):
        dead[t0:t0 + tokens_per_tile] = bool(dropped[t0:t0 + tokens_per_tile].all())
    return dead.to(DEV)


def _dead_elems(mask, rps, c):
    """bool [M, 8c]: the elements of a packed tensor of c channels per irrep that lie in dead tiles."""
    d = torch.zeros(len(mask) * rps, 8 * c, dtype=torch.bool, device=DEV)
    d[:, :4 * c] = _dead_rows(mask, rps, 128)[:, None]
    d[:, 4 * c:] = _dead_rows(mask, rps, 64)[:, None]
    return d


@functools.lru_cache(maxsize=None)
def _problem(cin, cout, M):
    """x, prepared weights, bias, column scales and a residual (made once per shape, never modified)."""
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(cin * 1000 + cout + M)
    x = torch.randn(M, 8 * cin, generator=g).to(torch.bfloat16).to(DEV)
    w32 = [(torch.randn(s, generator=g) * 0.1).to(DEV) for s in [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]]
    bias = torch.randn(cout, generator=g).to(DEV)
    cs = [torch.randn(n, generator=g).to(DEV) for n in [cout] * 4 + [2 * cout]]
    resid = torch.randn(M, 8 * cout, generator=g).to(DEV)
    wb, _ = ops.linear_prep(w32, None, cin, cout, torch.bfloat16, want_wb=True)
    return x, wb, bias, cs, resid


def _launch(x, wb, cin, cout, out_dtype, dropped=None, rps=0, bias=None, resid=None, rs=None, cs=None):
    from octic_vits_amd import ops
    M = x.shape[0]
    y = torch.full((M, 8 * cout), float("nan"), dtype=out_dtype, device=DEV)
    ops.linear_fwd(ops.pview(x, cin), wb, bias, ops.pview(y, cout), M, cin, cout, torch.bfloat16, out_dtype, x,
                   resid_v=None if resid is None else ops.pview(resid, cout), rs=rs, rps=rps if rs is not None else 1, cs5=cs,
                   dropped=dropped, dropped_rps=rps)
    torch.cuda.synchronize()
    return y


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("rps,B", SAMPLES)
@pytest.mark.parametrize("cin,cout,tile_n", SHAPES)
def test_plain_launch(cin, cout, tile_n, rps, B):
    from octic_vits_amd import _lib
    M = rps * B
    kernel, width, _, _ = _lib.plan("octic_linear_d8_plan", M, cin, cout, _lib.BF16, _lib.BF16, 0)
    assert kernel == _lib.LINEAR_RING and width == tile_n
    x, wb, _, _, _ = _problem(cin, cout, M)
    for name, mask in _masks(B).items():
        ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
        xz = x * (ss != 0).repeat_interleave(rps)[:, None].to(x.dtype)        # the contract: dropped samples' rows are zero
        ref = _launch(xz, wb, cin, cout, torch.bfloat16)
        xp = torch.where(_dead_elems(mask, rps, cin), torch.full_like(xz, float("nan")), xz)
        y = _launch(xp, wb, cin, cout, torch.bfloat16, dropped=ss, rps=rps)
        assert bool(torch.isfinite(y.float()).all()), (name, rps)
        assert torch.equal(y, ref), (name, rps)
        dead = _dead_elems(mask, rps, cout)
        assert bool((_bits(y)[dead] == 0).all()), (name, rps)
        if name == "all dropped":
            assert bool(dead.all())
        if name == "all kept":
            assert not bool(dead.any())


@pytest.mark.parametrize("rps,B", SAMPLES)
@pytest.mark.parametrize("cin,cout,tile_n", SHAPES)
def test_fused_launch(cin, cout, tile_n, rps, B):
    from octic_vits_amd import _lib
    M = rps * B
    kernel, width, fused, _ = _lib.plan("octic_linear_d8_plan", M, cin, cout, _lib.BF16, _lib.F32, 1)
    assert kernel == _lib.LINEAR_RING and width == tile_n and fused == 1
    x, wb, bias, cs, resid = _problem(cin, cout, M)
    for name, mask in _masks(B).items():
        ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
        ref = _launch(x, wb, cin, cout, torch.float32, rps=rps, bias=bias, resid=resid, rs=ss, cs=cs)
        xp = torch.where(_dead_elems(mask, rps, cin), torch.full_like(x, float("nan")), x)
        y = _launch(xp, wb, cin, cout, torch.float32, dropped=ss, rps=rps, bias=bias, resid=resid, rs=ss, cs=cs)
        assert torch.equal(y, ref), (name, rps)
        dead = _dead_elems(mask, rps, cout)
        assert torch.equal(_bits(y)[dead], _bits(resid)[dead]), (name, rps)


def test_bf16_residual_stream():
    """The fused instantiation with a bf16 output (a bf16 residual stream): eight columns per 16-byte piece."""
    cin, cout, rps, B = 640, 160, 37, 20
    x, wb, bias, cs, resid = _problem(cin, cout, rps * B)
    rb = resid.to(torch.bfloat16)
    mask = _masks(B)["bernoulli 1"]
    ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
    ref = _launch(x, wb, cin, cout, torch.bfloat16, rps=rps, bias=bias, resid=rb, rs=ss, cs=cs)
    xp = torch.where(_dead_elems(mask, rps, cin), torch.full_like(x, float("nan")), x)
    y = _launch(xp, wb, cin, cout, torch.bfloat16, dropped=ss, rps=rps, bias=bias, resid=rb, rs=ss, cs=cs)
    assert torch.equal(y, ref)
    dead = _dead_elems(mask, rps, cout)
    assert bool(dead.any()) and torch.equal(_bits(y)[dead], _bits(rb)[dead])


def test_the_w_stationary_kernel_computes_every_row():
    from octic_vits_amd import _lib
    cin, cout, rps, B = 160, 640, 37, 20
    M = rps * B
    assert _lib.plan("octic_linear_d8_plan", M, cin, cout, _lib.BF16, _lib.BF16, 0)[0] == _lib.LINEAR_WREG
    x, wb, _, _, _ = _problem(cin, cout, M)
    mask = _masks(B)["bernoulli 2"]
    ss = torch.tensor(mask, dtype=torch.float32, device=DEV)
    ref = _launch(x, wb, cin, cout, torch.bfloat16)
    assert torch.equal(_launch(x, wb, cin, cout, torch.bfloat16, dropped=ss, rps=rps), ref)   # non-zero rows: computed all the same


def test_refusals_through_ops():
    from octic_vits_amd import ops
    cin, cout, rps, B = 192, 96, 37, 3
    x, wb, bias, cs, resid = _problem(cin, cout, rps * B)
    ss = torch.full((B,), KEEP, device=DEV)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        _launch(x, wb, cin, cout, torch.bfloat16, dropped=ss, rps=rps, bias=bias)             # a plain masked launch with a bias
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        _launch(x, wb, cin, cout, torch.float32, dropped=ss, rps=rps, resid=resid)            # fused without rs
    with pytest.raises(ValueError):
        M = rps * B
        y = torch.empty(M, 8 * cout, dtype=torch.bfloat16, device=DEV)
        ops.linear_fwd(ops.pview(x, cin), wb, None, ops.pview(y, cout), M, cin, cout, torch.bfloat16, torch.bfloat16, x,
                       sample_scale=ss, skip_rps=rps, dropped=ss, dropped_rps=rps)            # two contracts for one mask


# ---- 4: a training step -----------------------------------------------------------------------------------------------
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
    """The same device-resident masks in every forward of a run (a captured step replays what it recorded)."""
    import octic_vits_amd.d8_layers as L
    calls, cache = [0], {}
    for k in range(16):                                              # made up front: nothing may be created while a step is captured
        g = torch.Generator().manual_seed(700 + k)
        cache[k] = (torch.bernoulli(torch.full((4,), 0.5), generator=g) * KEEP).to(DEV)
    cache[1] = torch.tensor([KEEP, 0.0, 0.0, KEEP], device=DEV)      # (two adjacent samples dropped: dead tiles in both groups)

    def source(B, keep, device):
        k = calls[0] % 16
        calls[0] += 1
        return cache[k]

    L.drop_path_mask_source = source
    yield calls
    L.drop_path_mask_source = None


@pytest.fixture
def ring_switch():
    import octic_vits_amd.functional as OF
    before = OF.RING_SKIP_DROPPED
    yield OF
    OF.RING_SKIP_DROPPED = before


@pytest.mark.parametrize("captured", [False, True])
def test_train_step_is_bitwise_with_and_without_the_ring_mask(captured, injected_masks, ring_switch, monkeypatch):
    """224 x 224 (T = 257), 4 images, two octic blocks and a standard one at embed_dim 512 (c = 64, 8 heads of 64): fc2 (K = 256)
    and the input gradients of fc1 (K = 256) and qkv (K = 192) run the ring kernel, proj + residual the W-stationary one."""
    from octic_vits_amd import _lib, ops
    from octic_vits_amd.train import Trainer, synthetic_batch
    M, c = 4 * 257, 64
    assert _lib.plan("octic_linear_d8_plan", M, 4 * c, c, _lib.BF16, _lib.F32, 1)[0] == _lib.LINEAR_RING      # fc2 + residual
    assert _lib.plan("octic_linear_d8_plan", M, 4 * c, c, _lib.BF16, _lib.BF16, 0)[0] == _lib.LINEAR_RING     # dgrad fc1
    assert _lib.plan("octic_linear_d8_plan", M, 3 * c, c, _lib.BF16, _lib.BF16, 0)[0] == _lib.LINEAR_RING     # dgrad qkv
    seen = [0]
    inner = ops.linear_fwd

    def counting(*a, **k):
        seen[0] += k.get("dropped") is not None
        return inner(*a, **k)

    monkeypatch.setattr(ops, "linear_fwd", counting)
    x, y = synthetic_batch(4, 10, DEV, seed=3, img_size=224)
    results = []
    for on in (True, False):
        ring_switch.RING_SKIP_DROPPED = on
        injected_masks[0] = 0
        seen[0] = 0
        tr = Trainer(_model(224, 512, 8, 3, 2), lr=1e-3)
        if captured:
            loss = tr.capture(x, y, warmup=1).replay(x, y).detach().clone()
        else:
            loss = tr.step(x, y).detach().clone()
            # per octic block: the two fused forwards (proj, fc2) and the input gradients of qkv and fc1
            assert seen[0] == (8 if on else 0), seen
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
