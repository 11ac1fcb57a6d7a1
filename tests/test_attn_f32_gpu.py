"""Float32 attention on the HIP engine (csrc/attn_f32.hip: exact-f32 MFMA, K / V or Q / dO streamed through LDS in blocks)
against float64 math on the CPU.

Tolerance: for the same float32 tensors the test measures the error of PyTorch's own CPU float32
scaled_dot_product_attention (and its autograd) against the float64 result - the reference implementation's error,
never the kernel's.  The kernel may err up to 4x that figure, floor 2e-6: the factor covers the online-softmax rescale
(one extra rounding per key block) and exp2 of a log2(e)-prescaled product, the floor T = 1 where the CPU error is 0.
Errors are max|got - ref| / max(1, max|ref|) per tensor.

Module-level routing checks compare the engine path with the SDPA path of the same module under the same bound, per
tensor: the floor 2e-6 for the octic model (the engine runs on the GPU only, so there is no CPU figure for it), and for
vit.Attention 4x the error of the same module on the CPU in float32 against float64, floor 2e-6.  Under fp16 autocast
the module's own SDPA path casts the octic q, k, v to fp16, which no float32 bound can meet - a property of that
comparison, not of the kernel - so there the issue's comparison is deliberately replaced: the SDPA side runs the octic
attention with autocast locally disabled (float32-accurate), the float32 half (the output of the last octic block) is
held to the floor 2e-6, and the tensors behind the fp16 standard block, which sit on the fp16 grid, may differ by two
fp16 ulps, 2 * 2^-10 of the tensor scale (a difference within the float32 bound can flip a rounding, and a flipped
value can flip the one computed from it)."""
import functools
import math
import types

import pytest
import torch

import cases

pytestmark = pytest.mark.gpu

B, H = 2, 3
FACTOR, FLOOR = 4.0, 2e-6


def _edge_tokens():
    from octic_vits_amd import ops
    rows, blk = ops.ATTN_F32_ROWS, ops.ATTN_F32_BLK
    ts = {1, 15, 16, 17, 33, 197, 257, 577}
    for c in (rows, blk):
        for m in range(c, 2 * rows + 1, c):
            ts |= {m - 1, m, m + 1}
    if max(ts) <= 4 * rows:
        ts.add(4 * rows + 33)
    return sorted(ts)


TOKENS = _edge_tokens()
SHAPES = [(T, hd) for T in TOKENS for hd in (16, 64, 80, 128)] + [(T, hd) for T in (65, 257) for hd in (48, 112)]
SHARP = [(T, hd) for T in TOKENS for hd in (64, 80)]


def _err(got, ref):
    ref = ref.double()
    return float((got.detach().cpu().double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


@functools.lru_cache(maxsize=4)
def _case(T, hd, qmul=1.0):
    """Seeded float32 tensors, the float64 reference and the CPU float32 reference error, computed once per shape."""
    g = torch.Generator().manual_seed(T * 131 + hd)
    q = 2 * qmul * torch.randn(B, H, T, hd, generator=g)
    k, v, do = (torch.randn(B, H, T, hd, generator=g) for _ in range(3))
    scale = hd ** -0.5
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    s = (q64 @ k64.transpose(-1, -2)) * scale
    o64 = torch.softmax(s, -1) @ v64
    ref = dict(zip(("dq", "dk", "dv"), torch.autograd.grad(o64, (q64, k64, v64), do.double())))
    ref["o"] = o64.detach()
    ref["lse"] = (torch.logsumexp(s, -1) / math.log(2.0)).detach()
    q32, k32, v32 = (t.clone().requires_grad_(True) for t in (q, k, v))
    o32 = torch.nn.functional.scaled_dot_product_attention(q32, k32, v32)
    cpu = dict(zip(("dq", "dk", "dv"), torch.autograd.grad(o32, (q32, k32, v32), do)))
    cpu["o"] = o32.detach()
    cpu["lse"] = torch.logsumexp((q @ k.transpose(-1, -2)) * scale, -1) / math.log(2.0)
    tol = {n: max(FACTOR * _err(cpu[n], ref[n]), FLOOR) for n in ref}
    return types.SimpleNamespace(q=q, k=k, v=v, do=do, scale=scale, ref=ref, tol=tol)


def _run(q, k, v, do, scale):
    """forward + backward of the kernels on device tensors -> dict of o, lse, dq, dk, dv"""
    from octic_vits_amd import ops
    o, lse = ops.attn_fwd(q, k, v, scale)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    ops.attn_bwd(q, k, v, o, do, lse, scale, dq, dk, dv)
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv)


def _check_case(T, hd, qmul):
    c = _case(T, hd, qmul)
    got = _run(*(t.cuda() for t in (c.q, c.k, c.v, c.do)), c.scale)
    torch.cuda.synchronize()
    bad = []
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.isfinite(got[n]).all(), n
        e = _err(got[n], c.ref[n])
        print(f"T={T} hd={hd} qmul={qmul} {n}: err {e:.3e} tol {c.tol[n]:.3e} ratio-to-cpu {e / (c.tol[n] / FACTOR):.2f}")
        if e > c.tol[n]:
            bad.append((n, e, c.tol[n]))
    assert not bad, bad


@pytest.mark.parametrize("T,hd", SHAPES)
def test_forward_and_backward_match_float64(T, hd):
    _check_case(T, hd, 1.0)


@pytest.mark.parametrize("T,hd", SHARP)
def test_sharp_softmax_matches_float64(T, hd):
    """q * 20: one key dominates a row, so the running-max rescale across key blocks decides the result."""
    _check_case(T, hd, 20.0)


@pytest.mark.parametrize("T", [17, 65, 257])
def test_nothing_past_row_T_is_read_or_written(T):
    """Operands and outputs are [:, :, :T] slices of NaN-filled [B,H,T+5,hd] buffers: finite, bitwise equal to the
    contiguous run, and the NaN tails of the output buffers stay NaN."""
    from octic_vits_amd import ops
    hd = 80
    c = _case(T, hd)
    dense = [t.cuda() for t in (c.q, c.k, c.v, c.do)]
    want = _run(*dense, c.scale)

    def padded(t=None):
        buf = torch.full((B, H, T + 5, hd), float("nan"), device="cuda")
        if t is not None:
            buf[:, :, :T] = t
        return buf

    qb, kb, vb, dob = (padded(t) for t in dense)
    ob, dqb, dkb, dvb = padded(), padded(), padded(), padded()
    q, k, v, do = (b[:, :, :T] for b in (qb, kb, vb, dob))
    o, lse = ops.attn_fwd(q, k, v, c.scale, out=ob[:, :, :T])
    ops.attn_bwd(q, k, v, o, do, lse, c.scale, dqb[:, :, :T], dkb[:, :, :T], dvb[:, :, :T])
    torch.cuda.synchronize()
    for name, buf in (("o", ob), ("dq", dqb), ("dk", dkb), ("dv", dvb)):
        assert torch.isfinite(buf[:, :, :T]).all(), name
        assert torch.equal(buf[:, :, :T], want[name]), name
        assert torch.isnan(buf[:, :, T:]).all(), name
    assert torch.equal(lse, want["lse"])


@pytest.mark.parametrize("Bq,T,Hq,hd", [(2, 197, 3, 64), (1, 257, 2, 80)])
def test_fused_projection_views_equal_the_head_major_run_bitwise(Bq, T, Hq, hd):
    """[B,T,3,H,hd] views through AttnFusedQKVFn in float32: forward and the single [B,T,3,H,hd] gradient are bitwise
    those of the [B,H,T,hd] run on permuted copies (the arithmetic does not depend on the strides)."""
    from octic_vits_amd.functional import AttnFusedQKVFn
    g = torch.Generator().manual_seed(T + hd)
    qkv = torch.randn(Bq, T, 3, Hq, hd, generator=g).cuda().requires_grad_(True)
    do = torch.randn(Bq, T, Hq * hd, generator=g).cuda()
    out = AttnFusedQKVFn.apply(qkv, hd ** -0.5)
    (dqkv,) = torch.autograd.grad(out, qkv, do)
    q, k, v = (qkv.detach()[:, :, i].permute(0, 2, 1, 3).contiguous() for i in range(3))
    want = _run(q, k, v, do.view(Bq, T, Hq, hd).permute(0, 2, 1, 3).contiguous(), hd ** -0.5)
    assert out.dtype == torch.float32 and dqkv.shape == qkv.shape
    assert torch.equal(out.view(Bq, T, Hq, hd).permute(0, 2, 1, 3), want["o"])
    for i, n in enumerate(("dq", "dk", "dv")):
        assert torch.equal(dqkv[:, :, i].permute(0, 2, 1, 3), want[n]), n


def test_bitwise_repeatable_and_graph_capture_equals_eager():
    c = _case(257, 80)
    dev = [t.cuda() for t in (c.q, c.k, c.v, c.do)]

    def step():
        r = _run(*dev, c.scale)
        return [r[n] for n in ("o", "lse", "dq", "dk", "dv")]

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
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, e1))


# ---- routing: float32 attention of the modules runs on the engine ---------------------------------------------------
def _product_ns():
    import octic_vits_amd.d8_invariantization as I
    import octic_vits_amd.d8_layers as L
    import octic_vits_amd.d8_utils as U
    import octic_vits_amd.model as M
    import octic_vits_amd.vit as V
    ns = types.SimpleNamespace()
    for mod in (U, I, L, M):
        for key, val in vars(mod).items():
            if not key.startswith("_"):
                setattr(ns, key, val)
    ns.Layer_scale_init_Block = V.Layer_scale_init_Block
    return ns


def _octic_model():
    """2-block hybrid_deit-style model (one octic block, one standard block; T = 65, head_dim 32) of the golden cases"""
    net = cases.build_model(_product_ns(), cases.CASES["model_global_pool"]["model"])
    return cases.fill_parameters(net).cuda().eval()


def _vit_attention():
    from octic_vits_amd.vit import Attention
    return cases.fill_parameters(Attention(384, num_heads=6, qkv_bias=True)).cuda()


def _image():
    return cases.randn("f32attn.img", 2, 3, 32, 32)


ROUTED = {                                                   # kind: (module, input, autocast dtype)
    "octic_f32": (_octic_model, _image, None),
    "vit_attention_f32": (_vit_attention, lambda: cases.randn("f32attn.tok", 2, 197, 384), None),
    "octic_fp16_autocast": (_octic_model, _image, torch.float16),
}
FP16_ULP2 = 2 * 2.0 ** -10


def _tensors(out):
    if hasattr(out, "packed"):
        return [out.packed]
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _tensors(o)]


def _forward_backward(mod, x0, cot, autocast=None):
    """[output, parameter gradients..., input gradient if there is one] as float tensors on the CPU"""
    for p in mod.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        out = mod(x)
    out.to(cot.dtype).backward(cot)
    grads = [p.grad for p in mod.parameters() if p.grad is not None]
    assert len(grads) >= 4
    if x.grad is not None:                           # token inputs; the patch embedding does not differentiate the image
        grads.append(x.grad)
    return [t.detach().cpu().clone() for t in [out] + grads]


def _cpu_reference_error(make, x0, cot):
    """error of the module on the CPU in float32 (its SDPA path) against float64, per result tensor"""
    r32 = _forward_backward(make().cpu(), x0.cpu(), cot.cpu())
    r64 = _forward_backward(make().cpu().double(), x0.cpu().double(), cot.cpu().double())
    return [_err(a, b) for a, b in zip(r32, r64)]


@pytest.mark.parametrize("kind", list(ROUTED))
def test_float32_attention_does_not_reach_sdpa(kind, monkeypatch):
    """With F.scaled_dot_product_attention patched to raise, the modules still run forward and backward in float32 and
    agree with their own SDPA path (ops.attn_f32_supported patched to False); bounds: the module docstring.  Under fp16
    autocast the standard block of the hybrid hands SDPA fp16 tensors - one of the cases that stay on SDPA - so there the
    patch raises for every call whose tensors are not fp16: the octic half's float32 attention may not reach it."""
    import torch.nn.functional as F
    from octic_vits_amd import ops
    make, inp, autocast = ROUTED[kind]
    mod = make()
    x0 = inp().cuda()
    with torch.no_grad():
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            cot = torch.randn(mod(x0).shape, generator=torch.Generator().manual_seed(7)).cuda()
    octic_half = []
    if autocast is not None:
        last = mod.blocks[mod.octic_equi_break_layer - 1]
        hook = last.register_forward_hook(lambda m, i, o: octic_half.append([t.detach().cpu() for t in _tensors(o)]))

    calls = []
    real = F.scaled_dot_product_attention

    def spy(*a, **k):
        calls.append(a[0].dtype)
        if a[0].dtype == torch.float32:              # the octic half: float32-accurate also under fp16 autocast
            with torch.autocast("cuda", enabled=False):
                return real(*a, **k)
        return real(*a, **k)

    def boom(*a, **k):
        if autocast is not None and a[0].dtype == torch.float16:
            return real(*a, **k)
        raise AssertionError(f"F.scaled_dot_product_attention reached with {a[0].dtype} tensors")

    with monkeypatch.context() as m:
        m.setattr(ops, "attn_f32_supported", lambda *a: False)
        m.setattr(F, "scaled_dot_product_attention", spy)
        want = _forward_backward(mod, x0, cot, autocast)
    assert torch.float32 in calls, "the comparison path must be the SDPA one"
    with monkeypatch.context() as m:
        m.setattr(F, "scaled_dot_product_attention", boom)
        got = _forward_backward(mod, x0, cot, autocast)
    assert len(got) == len(want)
    if autocast is not None:
        hook.remove()
        tols = [FP16_ULP2] * len(want)
        half_want, half_got = octic_half[-2], octic_half[-1]
        assert half_got and all(t.dtype == torch.float32 for t in half_got)
        for a, b in zip(half_got, half_want):
            e = _err(a, b)
            print(f"{kind}: octic half, engine-vs-SDPA difference {e:.3e} (bound {FLOOR:.3e})")
            assert e <= FLOOR, (kind, "octic half", e)
    elif kind == "vit_attention_f32":
        tols = [max(FACTOR * e, FLOOR) for e in _cpu_reference_error(make, x0, cot)]
    else:
        tols = [FLOOR] * len(want)
    bad = []
    for i, (a, b, tol) in enumerate(zip(got, want, tols)):
        assert torch.isfinite(a).all()
        e = _err(a, b)
        print(f"{kind}: tensor {i}, engine-vs-SDPA difference {e:.3e} (bound {tol:.3e})")
        if e > tol:
            bad.append((i, e, tol))
    assert not bad, (kind, bad)


def test_bf16_comparison_path_still_reaches_sdpa(monkeypatch):
    """The bf16 predicates patched to False (tests/test_attn_long_gpu.py's comparison path) still send a bf16 call to
    SDPA: the float32 predicate does not catch bf16 tensors."""
    import torch.nn.functional as F
    from octic_vits_amd import functional as OF, ops
    calls = []
    real = F.scaled_dot_product_attention

    def spy(*a, **k):
        calls.append(a[0].dtype)
        return real(*a, **k)

    q, k, v = (torch.randn(2, 2, 33, 64, device="cuda").bfloat16() for _ in range(3))
    monkeypatch.setattr(ops, "attn_supported", lambda *a: False)
    monkeypatch.setattr(ops, "attn_packed_ok", lambda *a: False)
    monkeypatch.setattr(F, "scaled_dot_product_attention", spy)
    o = OF.attention_core(q, k, v)
    assert calls == [torch.bfloat16] and o.dtype == torch.bfloat16


def test_attn_qkv_op_passes_opcheck_in_float32():
    from octic_vits_amd import dispatch  # noqa: F401  (registers torch.ops.octic)
    g = torch.Generator(device="cuda").manual_seed(2)
    qkv = (torch.randn(2, 65, 3, 2, 64, generator=g, device="cuda") * 0.5).requires_grad_(True)
    torch.library.opcheck(torch.ops.octic.attn_qkv, (qkv, 64 ** -0.5))


def test_no_score_matrix_is_allocated():
    """forward + backward at (8,16,577,64) raises the allocator's peak by less than one B H T T f32 score matrix"""
    Bm, Hm, T, hd = 8, 16, 577, 64
    q, k, v, do = (torch.randn(Bm, Hm, T, hd, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    r = _run(q, k, v, do, hd ** -0.5)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < Bm * Hm * T * T * 4
    assert torch.isfinite(r["dq"]).all()
