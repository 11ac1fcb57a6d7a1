"""Attention kernels that skip the samples a stochastic-depth mask drops (include/octic_hip.h: octic_attn_*_skip).

sample_scale[b] == 0 marks sample b as dropped: a kernel may skip it and then writes +0 to the sample's o rows and lse (forward) and
to its dq, dk, dv (backward).  All operands bf16, head_dim 80.  Output buffers that have an `out=` argument are pre-filled with NaN,
so an element no kernel wrote shows up; dout is random and non-zero for EVERY sample, so a zero gradient of a dropped sample proves
the kernel skipped it (the full computation would give non-zero values).

1. the headline routes (T = 257: a80::fwd_os_kernel and a80::bwd_kernel<8, true>), both layouts: kept samples bitwise the call
   without a mask, dropped samples all zeros; B = 70 walks the second 64-sample word of the kept / dropped lists;
2. the other routes (T = 258, 197, 37, 100, 321): kept samples bitwise, a dropped sample either zeros or bitwise;
3. a 2 octic + 2 standard block model (embed 320, 4 heads of 80, T = 257), forward + backward with the switch on and off, eagerly and as a captured step."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

HD, H = 80, 2
K = 2.0                       # 1 / keep at drop_path 0.5
NAMES = ("o", "lse", "dq", "dk", "dv")


@functools.lru_cache(maxsize=None)
def _operands(layout, B, T):
    g = torch.Generator().manual_seed(1000 * B + T + (7 if layout == "packed" else 0))
    if layout == "strided":
        qkv = torch.randn(B, T, 3, H, HD, generator=g).to(torch.bfloat16).cuda()
        do = torch.randn(B, T, H, HD, generator=g).to(torch.bfloat16).cuda()
    else:
        c = 10 * H
        qkv = (torch.randn(B, T, 3 * 8 * c, generator=g) * 0.7).to(torch.bfloat16).cuda()
        do = torch.randn(B, T, 8 * c, generator=g).to(torch.bfloat16).cuda()
    assert bool((do != 0).flatten(1).any(1).all())
    return qkv, do


def _run(layout, B, T, scale_list):
    """o, lse, dq, dk, dv (sample on dim 0) of one forward + backward with sample_scale = scale_list (None: no mask)."""
    from octic_vits_amd import ops
    qkv, do = _operands(layout, B, T)
    ss = None if scale_list is None else torch.tensor(scale_list, dtype=torch.float32, device="cuda")
    nan = float("nan")
    if layout == "strided":
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.full((B, T, H, HD), nan, dtype=torch.bfloat16, device="cuda")
        _, lse = ops.attn_fwd(q, k, v, HD ** -0.5, out=o.permute(0, 2, 1, 3), sample_scale=ss)
        dqkv = torch.full_like(qkv, nan)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        ops.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), do.permute(0, 2, 1, 3), lse, HD ** -0.5, dq, dk, dv, sample_scale=ss)
        return {"o": o, "lse": lse, "dq": dqkv[:, :, 0], "dk": dqkv[:, :, 1], "dv": dqkv[:, :, 2]}
    c = 10 * H
    o = torch.full((B, T, 8 * c), nan, dtype=torch.bfloat16, device="cuda")
    _, lse = ops.attn_fwd_packed(qkv, H, c, HD ** -0.5, out=o, sample_scale=ss)
    dqkv = ops.attn_bwd_packed(qkv, o, do, lse, H, c, HD ** -0.5, out=torch.full_like(qkv, nan), sample_scale=ss)
    # packed rows interleave q | k | v inside every irrep block (block width 3c): [B, T, 6 blocks.., 3, c]-like views per tensor
    cv = 3 * c
    one = dqkv[..., :4 * cv].reshape(B, T, 4, 3, c)
    two = dqkv[..., 4 * cv:].reshape(B, T, 2, 3, 2 * c)
    out = {"o": o, "lse": lse}
    for i, n in enumerate(("dq", "dk", "dv")):
        out[n] = torch.cat([one[:, :, :, i].flatten(2), two[:, :, :, i].flatten(2)], dim=-1)
    return out


@functools.lru_cache(maxsize=None)
def _unmasked(layout, B, T):
    ref = _run(layout, B, T, None)
    for n in NAMES:
        assert not torch.isnan(ref[n].float()).any(), n
    return ref


def _compare(got, ref, scale_list, must_skip):
    for n in NAMES:
        assert not torch.isnan(got[n].float()).any(), f"{n}: an element was never written"
        for b, sc in enumerate(scale_list):
            same = torch.equal(got[n][b], ref[n][b])
            if sc != 0.0:
                assert same, f"{n}: kept sample {b} differs from the call without a mask"
                continue
            zero = not bool(got[n][b].float().abs().max() > 0)
            if must_skip:
                assert zero, f"{n}: dropped sample {b} was computed (or holds stale values)"
            else:
                assert zero or same, f"{n}: dropped sample {b} is neither zeros nor the unmasked result"


B70 = [0.0] * 70
for _b in (0, 5, 62, 63, 64, 65, 69):
    B70[_b] = K

HEADLINE = {
    "b5_mixed": [K, 0.0, K, 0.0, 0.0],
    "b5_all_kept": [K] * 5,
    "b5_none_kept": [0.0] * 5,
    "b70_across_word": B70,
}


@pytest.mark.parametrize("pattern", sorted(HEADLINE))
@pytest.mark.parametrize("layout", ["strided", "packed"])
def test_headline_routes_skip_the_dropped_samples(layout, pattern):
    from octic_vits_amd import ops
    T = 257
    assert ops._attn_bwd_phases(T, HD)[0][0] == 3 and not ops.attn_streams(T, HD)       # fwd_os_kernel / bwd_kernel<8, true>
    scale_list = HEADLINE[pattern]
    B = len(scale_list)
    _compare(_run(layout, B, T, scale_list), _unmasked(layout, B, T), scale_list, must_skip=True)


@pytest.mark.parametrize("layout", ["strided", "packed"])
def test_non_zero_scales_give_the_null_pointer_result(layout):
    """Whatever the non-zero values (negative, tiny, huge): nothing is skipped, every tensor is bitwise the call without a mask."""
    scale_list = [0.5, -1.0, 1e-30, 3e38, 2.0]
    got, ref = _run(layout, 5, 257, scale_list), _unmasked(layout, 5, 257)
    for n in NAMES:
        assert torch.equal(got[n], ref[n]), n


@pytest.mark.parametrize("T", [258, 197, 37, 100, 321])
@pytest.mark.parametrize("layout", ["strided", "packed"])
def test_other_routes_keep_the_contract(layout, T):
    scale_list = [K, 0.0, K]
    _compare(_run(layout, 3, T, scale_list), _unmasked(layout, 3, T), scale_list, must_skip=False)


# ---- 3: end to end ---------------------------------------------------------------------------------------------------

# 224 x 224 at patch 14: T = 257; head_dim 80.  The octic row kernels take c = embed_dim / 8 channels per irrep in multiples of 8
# and the packed attention c = 10 heads, so the smallest such model is 4 heads x 80 = 320 (160 = 2 heads is refused: c = 20).
_KW = dict(img_size=224, patch_size=14, num_classes=10, embed_dim=320, depth=4, num_heads=4, qkv_bias=True,
           init_scale=0.1, drop_path_rate=0.5, octic_equi_break_layer=2)
# per forward: attention and MLP branch of octic block 0, 1, standard block 0, 1 - one attention branch drops everybody, one
# keeps everybody
_MASKS = [[1, 0, 1, 0], [1, 1, 0, 0],
          [0, 0, 0, 0], [0, 1, 0, 1],
          [1, 1, 1, 1], [1, 0, 0, 1],
          [0, 1, 1, 0], [0, 0, 1, 1]]


def _model():
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(0)
    return OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                  **_KW).cuda()


@pytest.fixture
def injected_masks():
    """The same eight device-resident masks in every forward (a captured step replays what it recorded)."""
    import octic_vits_amd.d8_layers as L
    masks = [torch.tensor(m, dtype=torch.float32, device="cuda") for m in _MASKS]
    calls = [0]

    def source(B, keep, device):
        m = masks[calls[0] % len(masks)]
        calls[0] += 1
        assert B == m.numel()
        return m

    L.drop_path_mask_source = source
    yield calls
    L.drop_path_mask_source = None


@pytest.fixture
def skip_switch():
    import octic_vits_amd.functional as OF
    before = OF.ATTN_SKIP_DROPPED
    yield OF
    OF.ATTN_SKIP_DROPPED = before


def _count_masked_calls(monkeypatch):
    from octic_vits_amd import ops
    seen = {"packed": 0, "strided": 0}
    fp, fs = ops.attn_fwd_packed, ops.attn_fwd

    def packed(*a, **k):
        seen["packed"] += k.get("sample_scale") is not None
        return fp(*a, **k)

    def strided(*a, **k):
        seen["strided"] += k.get("sample_scale") is not None
        return fs(*a, **k)

    monkeypatch.setattr(ops, "attn_fwd_packed", packed)
    monkeypatch.setattr(ops, "attn_fwd", strided)
    return seen


def test_hybrid_model_forward_backward_is_bitwise_with_and_without_skipping(injected_masks, skip_switch, monkeypatch):
    from octic_vits_amd.train import synthetic_batch
    seen = _count_masked_calls(monkeypatch)
    net = _model().train()
    x, y = synthetic_batch(4, 10, "cuda", 3)
    results = []
    for on in (True, False):
        skip_switch.ATTN_SKIP_DROPPED = on
        injected_masks[0] = 0
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = net(x)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits.float(), y)
        loss.backward()
        results.append((logits.detach().clone(), loss.detach().clone(),
                        {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
        if on:
            assert seen == {"packed": 2, "strided": 2}, seen       # both octic and both standard blocks handed their mask on
    assert seen == {"packed": 2, "strided": 2}, seen               # ... and none of them with the switch off
    (la, sa, ga), (lb, sb, gb) = results
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    assert set(ga) == set(gb) and len(ga) > 20
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_captured_step_with_skipping_equals_eager_steps(injected_masks, skip_switch):
    """Trainer.capture (two eager warm-up steps, then two replays) against four eager steps: the kept / dropped lists are built
    inside the kernels from the recorded mask tensors, so the graph holds nothing that depends on the kept count."""
    from octic_vits_amd.train import Trainer, synthetic_batch
    skip_switch.ATTN_SKIP_DROPPED = True
    batches = [synthetic_batch(4, 10, "cuda", s) for s in range(3)]
    out = []
    for graphed in (False, True):
        injected_masks[0] = 0
        tr = Trainer(_model(), lr=1e-3)
        if graphed:
            gs = tr.capture(*batches[0], warmup=2)
            losses = [float(gs.replay(*batches[i])) for i in (1, 2)]
        else:
            for _ in range(2):
                tr.step(*batches[0])
            losses = [float(tr.step(*batches[i]).detach()) for i in (1, 2)]
        out.append((losses, [p.detach().clone() for p in tr.raw_model.parameters()]))
    (la, pa), (lb, pb) = out
    assert la == lb, (la, lb)
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
