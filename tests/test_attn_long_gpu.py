"""Long-sequence attention (csrc/attn_stream.hip: K / V, or Q / dO, streamed through LDS in blocks of 64 rows) against
fp32 / fp64 references, the existing kernel family, and the model paths that reach it (T > 320: DeiT-III at 384^2,
ViT-H/14 at 448^2).  Tolerances as in test_attention_gpu.py: outputs 2e-2 (bf16 outputs, P rounded to bf16 before P V),
lse 2e-3, gradients 3e-2 of the gradient scale."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _ref(q, k, v, scale):
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    lse2 = torch.logsumexp(s, dim=-1) / math.log(2.0)
    return torch.softmax(s, dim=-1) @ v.float(), lse2


def _ref_grads(q, k, v, do, scale):
    q, k, v = (t.float().detach().requires_grad_(True) for t in (q, k, v))
    o = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    o.backward(do.float())
    return q.grad, k.grad, v.grad


def _grads_close(pairs):
    for name, got, want in pairs:
        scale = max(1.0, float(want.abs().max()))
        err = float((got.float() - want).abs().max())
        assert err <= 3e-2 * scale, f"{name}: max err {err:.3e} (scale {scale:.3g})"


class _stream_route:
    """ROUTE_ATTN_STREAM = value for the body (1: the streaming kernels at every T)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        from octic_vits_amd import _lib
        self.old = _lib.route_override(_lib.ROUTE_ATTN_STREAM, self.value)

    def __exit__(self, *exc):
        from octic_vits_amd import _lib
        _lib.route_override(_lib.ROUTE_ATTN_STREAM, self.old)


SHAPES = [(2, 2, 321, 80), (1, 3, 577, 64), (1, 2, 1025, 80), (1, 1, 1370, 80), (1, 2, 700, 128), (2, 1, 333, 16),
          (1, 1, 2049, 64)]


@pytest.mark.parametrize("qmul", [1.0, 20.0])
@pytest.mark.parametrize("B,H,T,hd", SHAPES)
def test_stream_fwd_matches_reference(B, H, T, hd, qmul):
    """qmul = 20: sharp softmax, the running-max rescale across key blocks matters."""
    from octic_vits_amd import ops
    g = torch.Generator().manual_seed(T * 131 + hd)
    q, k, v = (torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16).cuda() for _ in range(3))
    q = (q.float() * qmul).bfloat16()
    scale = hd ** -0.5
    o, lse = ops.attn_fwd(q, k, v, scale)
    ro, rl = _ref(q, k, v, scale)
    tol = 2e-2 if qmul == 1.0 else 3e-2
    assert torch.isfinite(o.float()).all()
    assert torch.allclose(o.float(), ro, atol=tol, rtol=tol), (o.float() - ro).abs().max()
    assert torch.allclose(lse, rl, atol=2e-3 * max(1.0, qmul / 4), rtol=1e-4), (lse - rl).abs().max()


@pytest.mark.parametrize("B,H,T,hd", SHAPES)
def test_stream_bwd_matches_reference(B, H, T, hd):
    from octic_vits_amd.functional import AttnFn
    g = torch.Generator().manual_seed(T * 17 + hd)
    q, k, v = (torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16).cuda().requires_grad_(True) for _ in range(3))
    do = torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16).cuda()
    o = AttnFn.apply(q, k, v, hd ** -0.5)
    o.backward(do)
    rq, rk, rv = _ref_grads(q, k, v, do, hd ** -0.5)
    _grads_close((("dq", q.grad, rq), ("dk", k.grad, rk), ("dv", v.grad, rv)))


def test_stream_strided_views_of_a_fused_qkv_tensor():
    """[B,T,3,H,hd] views (the standard block's layout) through AttnFusedQKVFn at T = 577, forward and backward."""
    from octic_vits_amd.functional import AttnFusedQKVFn
    B, T, H, hd = 2, 577, 4, 64
    g = torch.Generator().manual_seed(9)
    qkv = torch.randn(B, T, 3, H, hd, generator=g).to(torch.bfloat16).cuda().requires_grad_(True)
    do = torch.randn(B, T, H * hd, generator=g).to(torch.bfloat16).cuda()
    out = AttnFusedQKVFn.apply(qkv, hd ** -0.5)
    out.backward(do)
    ref = qkv.detach().float().requires_grad_(True)
    q, k, v = (ref[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ro = (torch.softmax((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1) @ v).transpose(1, 2).reshape(B, T, H * hd)
    ro.backward(do.float())
    assert torch.allclose(out.float(), ro, atol=2e-2, rtol=2e-2)
    _grads_close((("dqkv", qkv.grad, ref.grad),))


@pytest.mark.parametrize("T", [321, 577, 1025])
@pytest.mark.parametrize("w", [10, 8])
def test_stream_packed_matches_pack_attention_unpack(T, w):
    """Packed rows (HeadMap gathers) against pack -> strided streaming kernels -> unpack: same arithmetic per head in a
    different element order inside the dot products."""
    from octic_vits_amd import functional as OF, ops
    B, H = 2, 16
    c, hd = w * H, 8 * w
    torch.manual_seed(B * 1000 + T + w)
    qkv = (torch.randn(B, T, 3 * 8 * c, device="cuda") * 0.7).bfloat16().requires_grad_(True)
    do = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    assert ops.attn_packed_ok(T, c, H, qkv.dtype)
    o1 = OF.AttnPackedFn.apply(qkv, H, c, hd ** -0.5)
    (g1,) = torch.autograd.grad(o1, qkv, do)
    q, k, v = OF.PackHeadsFn.apply(qkv, H, c)
    o2 = OF.UnpackHeadsFn.apply(OF.AttnFn.apply(q, k, v, hd ** -0.5), c)
    (g2,) = torch.autograd.grad(o2, qkv, do)
    for a, b, name in ((o1, o2, "o"), (g1, g2, "dqkv")):
        a, b = a.float(), b.float()
        err = (a - b).abs().max().item()
        assert err <= 2e-2 * b.abs().max().item() + 1e-3, (name, err, b.abs().max().item())
        assert ((a - b).norm() / b.norm()).item() < 1e-2, name


@pytest.mark.parametrize("T,w", [(577, 8), (1025, 10), (321, 10)])
def test_stream_packed_matches_fp64_reference(T, w):
    """Packed rows against the oracle's AttentionD8 core in float64: oracle.pack_heads -> softmax attention ->
    oracle.unpack_heads, forward and backward (mirrors test_packed_attention_matches_fp64_reference)."""
    sys.path.insert(0, ROOT)
    from oracle import octic_ref as R
    from octic_vits_amd import functional as OF
    B, H = 1, 16
    c, hd = w * H, 8 * w
    cv = 3 * c
    torch.manual_seed(T + w)
    qkv = (torch.randn(B, T, 3 * 8 * c, device="cuda") * 0.7).bfloat16().requires_grad_(True)
    do = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    o = OF.AttnPackedFn.apply(qkv, H, c, hd ** -0.5)
    (g,) = torch.autograd.grad(o, qkv, do)
    x = qkv.detach().float().cpu().double().requires_grad_(True)
    tup = tuple(x[..., i * cv:(i + 1) * cv] for i in range(4)) + (x[..., 4 * cv:].reshape(B, T, 2, 2 * cv),)
    q, k, v = R.pack_heads(tup, H)
    p = torch.softmax(q @ k.transpose(-1, -2) * hd ** -0.5, -1)
    out5 = R.unpack_heads(p @ v)
    ref = torch.cat(list(out5[:4]) + [out5[4].flatten(-2)], dim=-1)
    (gref,) = torch.autograd.grad(ref, x, do.float().cpu().double())
    for got, want, name in ((o, ref, "o"), (g, gref, "dqkv")):
        got, want = got.detach().float().cpu().double(), want.detach()
        err = (got - want).abs().max().item()
        assert err <= 2e-2 * want.abs().max().item(), (name, err)
        assert ((got - want).norm() / want.norm()).item() < 1e-2, name


@pytest.mark.parametrize("T,hd", [(197, 64), (257, 80)])
def test_stream_knob_at_vit_token_counts_agrees_with_the_resident_kernels(T, hd):
    """OCTIC_ROUTE_ATTN_STREAM = 1 runs the streaming kernels at T <= 320: they agree with the resident family and with
    the fp32 reference, strided and packed."""
    from octic_vits_amd import functional as OF, ops
    B, H = 2, 16
    g = torch.Generator().manual_seed(T + hd)
    q, k, v = (torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16).cuda().requires_grad_(True) for _ in range(3))
    do = torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16).cuda()

    def run():
        o = OF.AttnFn.apply(q, k, v, hd ** -0.5)
        return (o,) + torch.autograd.grad(o, (q, k, v), do)

    base = run()
    with _stream_route(1):
        assert ops.attn_streams(T, hd)
        got = run()
    assert not ops.attn_streams(T, hd)
    ro, _ = _ref(q, k, v, hd ** -0.5)
    assert torch.allclose(got[0].float(), ro, atol=2e-2, rtol=2e-2)
    assert torch.allclose(got[0].float(), base[0].float(), atol=2e-2, rtol=2e-2)
    rq, rk, rv = _ref_grads(q, k, v, do, hd ** -0.5)
    _grads_close((("dq", got[1], rq), ("dk", got[2], rk), ("dv", got[3], rv)))
    _grads_close((("dq/base", got[1], base[1].float()), ("dk/base", got[2], base[2].float()),
                  ("dv/base", got[3], base[3].float())))
    # packed rows
    c = hd // 8 * H
    torch.manual_seed(T)
    qkv = (torch.randn(B, T, 3 * 8 * c, device="cuda") * 0.7).bfloat16().requires_grad_(True)
    dop = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    o1 = OF.AttnPackedFn.apply(qkv, H, c, hd ** -0.5)
    (g1,) = torch.autograd.grad(o1, qkv, dop)
    with _stream_route(1):
        o2 = OF.AttnPackedFn.apply(qkv, H, c, hd ** -0.5)
        (g2,) = torch.autograd.grad(o2, qkv, dop)
    for a, b, name in ((o2, o1, "o"), (g2, g1, "dqkv")):
        a, b = a.float(), b.float()
        assert (a - b).abs().max().item() <= 2e-2 * b.abs().max().item() + 1e-3, name


def test_stream_is_bitwise_repeatable_and_graph_capture_equals_eager():
    """No atomics, one writer per gradient element, fixed order: two eager runs and a hipGraph replay of forward + backward
    at T = 1025 (packed, head_dim 80) are bit-for-bit equal."""
    from octic_vits_amd import ops
    B, H, T, c = 2, 16, 1025, 160
    torch.manual_seed(5)
    qkv = (torch.randn(B, T, 24 * c, device="cuda") * 0.7).bfloat16()
    do = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    sc = 80 ** -0.5

    def step():
        o, lse = ops.attn_fwd_packed(qkv, H, c, sc)
        return o, ops.attn_bwd_packed(qkv, o, do, lse, H, c, sc)

    e1 = step()
    e2 = step()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(e1, e2))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, e1))


@pytest.mark.parametrize("kind", ["d8", "standard"])
def test_long_attention_modules_do_not_reach_sdpa(kind, monkeypatch):
    """AttentionD8 and the standard Attention at T = 577 under bf16 autocast: with SDPA patched to raise they still run
    (HIP kernels only) and agree with their SDPA path (attn_supported / attn_packed_ok patched to False) within bf16
    tolerance."""
    import torch.nn.functional as F
    from octic_vits_amd import ops
    from octic_vits_amd.d8_layers import AttentionD8
    from octic_vits_amd.functional import Octic
    from octic_vits_amd.vit import Attention
    B, T, D, H = 2, 577, 512, 8
    torch.manual_seed(3)
    if kind == "d8":
        mod = AttentionD8(D, num_heads=H, qkv_bias=True).cuda()
        fwd = lambda t: mod(Octic(t, D // 8)).packed
    else:
        mod = Attention(D, num_heads=H, qkv_bias=True).cuda()
        fwd = mod
    x0 = torch.randn(B, T, D, device="cuda")
    do = torch.randn(B, T, D, device="cuda")

    def run():
        for p in mod.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = fwd(x)
        out.float().backward(do)
        return out.detach().float(), x.grad.float(), [p.grad.detach().float().clone() for p in mod.parameters()]

    with monkeypatch.context() as m:
        m.setattr(ops, "attn_supported", lambda *a: False)
        m.setattr(ops, "attn_packed_ok", lambda *a: False)
        want = run()

    def boom(*a, **k):
        raise AssertionError("F.scaled_dot_product_attention reached")
    with monkeypatch.context() as m:
        m.setattr(F, "scaled_dot_product_attention", boom)
        got = run()
    (o_g, dx_g, pg_g), (o_w, dx_w, pg_w) = got, want
    assert (o_g - o_w).abs().max().item() <= 2e-2 * max(1.0, o_w.abs().max().item())
    assert ((dx_g - dx_w).norm() / dx_w.norm()).item() < 2e-2
    for a, b in zip(pg_g, pg_w):
        assert ((a - b).norm() / b.norm().clamp_min(1e-12)).item() < 2e-2


def test_attn_packed_op_passes_opcheck_at_577_tokens():
    from octic_vits_amd import dispatch  # noqa: F401  (registers torch.ops.octic)
    H, c = 16, 128
    qkv = (torch.randn(2, 577, 24 * c, device="cuda") * 0.7).bfloat16()
    torch.library.opcheck(torch.ops.octic.attn_packed.default, (qkv, H, c, 64 ** -0.5))


def _deit_pair(name, img_size, depth=2):
    """reduced-depth model through the same constructor arguments as deit_models (and the oracle's equivalent)."""
    sys.path.insert(0, ROOT)
    from oracle import octic_ref as R
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    p, D = {"hybrid_deit_large_patch16": (16, 1024), "hybrid_deit_huge_patch14": (14, 1280)}[name]
    kw = dict(img_size=img_size, patch_size=p, embed_dim=D, depth=depth, num_heads=16, mlp_ratio=4, qkv_bias=True,
              num_classes=1000)
    ref = cases.fill_parameters(R.OcticVisionTransformer(octic_block_layers=R.Layer_scale_init_BlockD8,
                                                         standard_block_layers=R.Layer_scale_init_Block, **kw),
                                salt="long.")
    net = OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                 **kw)
    net.load_state_dict(ref.state_dict(), strict=True)
    return ref, net.cuda()


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("name,img_size,T", [("hybrid_deit_large_patch16", 384, 577), ("hybrid_deit_huge_patch14", 448, 1025)])
def test_long_sequence_model_step_matches_the_oracle(name, img_size, T):
    """One bf16-autocast forward + backward of the reduced-depth model at its long-sequence resolution against the CPU
    oracle in f32; per-tensor relative L2 of the gradients within max(3e-2, 2 x the oracle's own distance under CPU bf16
    autocast) - the yardstick of test_hybrid_vit_huge_train_step_at_the_bench_batch_matches_the_oracle.  Catches any
    kernel on the path that assumed T <= 320."""
    ref, net = _deit_pair(name, img_size)
    assert (img_size // net.patch_embed.patch_size[0]) ** 2 + 1 == T
    B = 2
    img = cases.randn("long.img", B, 3, img_size, img_size)
    cot = cases.randn("long.cot", B, 1000)
    torch.set_num_threads(min(32, torch.get_num_threads()))
    names = [n for n, p in ref.named_parameters() if p.requires_grad]
    params = dict(ref.named_parameters())
    ref.train()

    def oracle(autocast):
        for p in ref.parameters():
            p.grad = None
        if autocast:
            with torch.autocast("cpu", dtype=torch.bfloat16):
                out = ref(img)
        else:
            out = ref(img)
        (out.float() * cot).sum().backward()
        return out.detach().float(), {n: params[n].grad.detach().double().numpy().copy() for n in names}

    _, g_bf = oracle(True)
    want, g_ref = oracle(False)
    net.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(img.cuda())
    (out.float() * cot.cuda()).sum().backward()
    assert (out.float().cpu() - want).abs().max().item() <= 5e-2 * max(1.0, want.abs().max().item())
    got = dict(net.named_parameters())
    bad = []
    for n in names:
        w = g_ref[n]
        den = max(float(np.linalg.norm(w)), 1e-12)
        yard = float(np.linalg.norm(g_bf[n] - w)) / den
        rel = float(np.linalg.norm(got[n].grad.detach().float().cpu().double().numpy() - w)) / den
        if rel > max(3e-2, 2.0 * yard):
            bad.append((n, rel, yard))
    assert not bad, bad[:8]


def test_graphed_forward_at_577_tokens_equals_eager_bitwise():
    from octic_vits_amd.serve import GraphedForward
    _, net = _deit_pair("hybrid_deit_large_patch16", 384)
    x = cases.randn("long.serve", 2, 3, 384, 384).cuda()
    net.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        eager = net(x).float()
    gf = GraphedForward(net, x)
    got = gf(x).float()
    torch.cuda.synchronize()
    assert torch.equal(got, eager)
