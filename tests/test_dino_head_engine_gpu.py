"""The DINO / iBOT head on the HIP engine (csrc/dino_norm.hip, functional.dino_head_forward, ssl.DINO_HEAD_HIP) on the device:
the L2-normalisation and weight-norm kernels at the smallest shapes that reach every code path (one chunk per lane, a partial
wave, several chunk slots, the widest row; one row, a partial workgroup, more than one workgroup; a tail tile of the transposed
store), the whole head against a float64 run of the stock module, freshness, routing and the training step.

The accuracy rule is the project's (NOTES 'DINO head'): against float64 the engine may be off by at most twice the stock arm's
own error on the same inputs plus one ulp of the output dtype, in the max norm, the ulp taken at the largest reference value.

Nothing here captures a graph or uses a side stream (tests/test_dino_head_engine_host.py says why)."""
import contextlib
import math
import os
import random
import subprocess
import sys
import warnings

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
EPS = 1e-12


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g, device="cuda").to(dtype)


def _ulp(dtype, magnitude):
    """One unit in the last place of `dtype` at |value| = magnitude."""
    if magnitude == 0.0 or not math.isfinite(magnitude):
        return 0.0
    return torch.finfo(dtype).eps * 2.0 ** math.floor(math.log2(magnitude))


def _rule(name, got, stock, ref64, dtype=None):
    """max |got - ref| <= 2 max |stock - ref| + 1 ulp(dtype) at max |ref|; every figure is printed first."""
    dtype = dtype or got.dtype
    ref64 = ref64.double()
    e_got = float((got.double() - ref64).abs().max())
    e_stock = float((stock.double() - ref64).abs().max())
    top = float(ref64.abs().max())
    bound = 2.0 * e_stock + _ulp(dtype, top)
    print(f"{name}: engine err {e_got:.3e}  stock err {e_stock:.3e}  max|ref| {top:.3e}  bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert e_got <= bound, (name, e_got, e_stock, bound)


@contextlib.contextmanager
def _switch(value):
    from octic_vits_amd import ssl as S
    old, S.DINO_HEAD_HIP = S.DINO_HEAD_HIP, value
    try:
        yield
    finally:
        S.DINO_HEAD_HIP = old


def _timed(fn):
    from octic_vits_amd import ops
    ops.KERNEL_TIMER.enable()
    try:
        out = fn()
        names = {r[0] for r in ops.KERNEL_TIMER.records}
    finally:
        ops.KERNEL_TIMER.disable()
        ops.KERNEL_TIMER.records = []
    return out, names


# ------------------------------------------------------------------------------------------------------------ L2 norm
L2_D = [8, 64, 256, 264, 4096]
L2_ROWS = [1, 7, 64, 65]


def _pow2_rows(g, rows, D, dtype):
    """Rows whose norm is an exact power of two whatever the summation order: one entry 2^(m-1) and twelve 2^(m-2) (sum of
    squares 4^m), or four entries 2^(m-1) where the row is too short; random places, signs and m."""
    x = torch.zeros(rows, D, device="cuda")
    for r in range(rows):
        m = int(torch.randint(-6, 7, (1,), generator=g, device="cuda"))
        n = 13 if D >= 13 else 4
        pos = torch.randperm(D, generator=g, device="cuda")[:n]
        sign = torch.randint(0, 2, (n,), generator=g, device="cuda").float() * 2 - 1
        mag = torch.full((n,), 2.0 ** (m - 2), device="cuda") if n == 13 else torch.full((n,), 2.0 ** (m - 1), device="cuda")
        if n == 13:
            mag[0] = 2.0 ** (m - 1)
        x[r, pos] = sign * mag
    return x.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", L2_ROWS)
@pytest.mark.parametrize("D", L2_D)
def test_l2norm_power_of_two_norms_equal_stock_bitwise(D, rows, dtype):
    from octic_vits_amd import ops
    x = _pow2_rows(_gen(D * 100 + rows), rows, D, dtype)
    y, inv = ops.l2norm_rows(x, EPS)
    want = F.normalize(x, dim=-1, p=2, eps=EPS)
    assert y.dtype == dtype and torch.equal(y, want)
    assert torch.equal(inv, 1.0 / x.float().norm(dim=-1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", L2_ROWS)
@pytest.mark.parametrize("D", L2_D)
def test_l2norm_general_rows_against_float64(D, rows, dtype):
    from octic_vits_amd import functional as OF, ops
    g = _gen(D * 1000 + rows)
    x = (_randn(g, rows, D) * (0.1 + 3.0 * torch.rand(rows, 1, generator=g, device="cuda"))).to(dtype)
    cot = _randn(g, rows, D, dtype=dtype)
    leaf = x.clone().requires_grad_(True)
    # the stock arm as autocast runs it: the norm and the division in f32 (autocast casts `norm` up and bf16 / f32 promotes),
    # ONE rounding to the output dtype - not bf16 F.normalize, whose bf16 norm would double the stock error and the bound
    with torch.autocast("cuda", dtype=torch.bfloat16):
        stock = F.normalize(leaf, dim=-1, p=2, eps=EPS)
    assert stock.dtype == torch.float32
    stock.backward(cot.float())
    stock = stock.to(dtype)
    leaf64 = x.double().requires_grad_(True)
    ref = F.normalize(leaf64, dim=-1, p=2, eps=EPS)
    ref.backward(cot.double())
    mine = x.clone().requires_grad_(True)
    y = OF.L2NormRowsFn.apply(mine, EPS)
    y.backward(cot)
    assert y.dtype == dtype and mine.grad.dtype == dtype
    _rule("y", y.detach(), stock.detach(), ref.detach())
    _rule("dx", mine.grad, leaf.grad, leaf64.grad)
    # the functions under the node: same bits, and inv is the f32 reciprocal norm
    y2, inv = ops.l2norm_rows(x, EPS)
    assert torch.equal(y2, y.detach())
    torch.testing.assert_close(inv.double(), 1.0 / x.double().norm(dim=-1), rtol=2.0 ** -20, atol=0)
    assert torch.equal(ops.l2norm_rows_bwd(cot, x, inv, EPS), mine.grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_l2norm_zero_tiny_and_nan_rows(dtype):
    """An exactly zero row and a row below eps against the float64 formulas, forward and backward (clamp_min passes no gradient:
    dx = g / eps there); a NaN row leaves its neighbours bitwise unchanged.  Tolerances from the formats: the f32 sum of 264
    squares, the square root and the division are a handful of roundings (2^-20 relative is 16 f32 ulps), the output rounding
    is half an ulp of `dtype`; the projection g - yh (yh . g) cancels, so dx is bounded relative to the row's max |g| / norm."""
    from test_dino_head_engine_host import l2norm_formulas
    from octic_vits_amd import ops
    g = _gen(17)
    D = 264
    x = _randn(g, 9, D)
    x[2] = 0.0
    x[5] = 1e-15 * _randn(g, D)
    x[7] *= 1e-9
    x = x.to(dtype)
    cot = _randn(g, 9, D, dtype=dtype)
    assert float(x[5].double().norm()) < EPS < float(x[7].double().norm())
    y, inv = ops.l2norm_rows(x, EPS)
    dx = ops.l2norm_rows_bwd(cot, x, inv, EPS)
    y64, inv64, dx64 = l2norm_formulas(x.double(), cot.double(), EPS)
    rt = 2.0 ** -20 + torch.finfo(dtype).eps / 2
    torch.testing.assert_close(inv.double(), inv64[:, 0], rtol=2.0 ** -20, atol=0)
    torch.testing.assert_close(y.double(), y64, rtol=rt, atol=0)
    assert float(y[2].abs().max()) == 0.0 and float(inv[2]) == float(torch.tensor(1.0 / EPS, dtype=torch.float32))
    for r in range(9):
        scale = float(cot[r].double().abs().max() * inv64[r, 0])
        torch.testing.assert_close(dx[r].double(), dx64[r], rtol=rt, atol=(2.0 ** -17 + torch.finfo(dtype).eps) * scale)
    for r in (2, 5):                                                  # clamped rows: g * inv, one product, one rounding
        torch.testing.assert_close(dx[r].double(), cot[r].double() * inv64[r], rtol=rt, atol=0)
    # NaN stays in its row
    xn = x.clone()
    xn[4, 3] = float("nan")
    yn, invn = ops.l2norm_rows(xn, EPS)
    dxn = ops.l2norm_rows_bwd(cot, xn, invn, EPS)
    keep = [r for r in range(9) if r != 4]
    assert bool(torch.isnan(yn[4]).all()) and bool(torch.isnan(dxn[4]).all()) and bool(torch.isnan(invn[4]))
    assert torch.equal(yn[keep], y[keep]) and torch.equal(dxn[keep], dx[keep]) and torch.equal(invn[keep], inv[keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [64, 264, 4096])
def test_l2norm_is_repeatable_and_rows_ignore_their_batch_mates(D, dtype):
    from octic_vits_amd import ops
    g = _gen(D)
    x, cot = _randn(g, 65, D, dtype=dtype), _randn(g, 65, D, dtype=dtype)
    y, inv = ops.l2norm_rows(x, EPS)
    dx = ops.l2norm_rows_bwd(cot, x, inv, EPS)
    y2, inv2 = ops.l2norm_rows(x, EPS)
    assert torch.equal(y, y2) and torch.equal(inv, inv2) and torch.equal(dx, ops.l2norm_rows_bwd(cot, x, inv, EPS))
    for r in (0, 37, 64):                                             # alone, and at another place among other rows
        y1, inv1 = ops.l2norm_rows(x[r:r + 1].clone(), EPS)
        assert torch.equal(y1[0], y[r]) and torch.equal(inv1[0], inv[r])
        assert torch.equal(ops.l2norm_rows_bwd(cot[r:r + 1].clone(), x[r:r + 1].clone(), inv1, EPS)[0], dx[r])
    other, ocot = _randn(g, 7, D, dtype=dtype), _randn(g, 7, D, dtype=dtype)
    other[3], ocot[3] = x[37], cot[37]
    yo, invo = ops.l2norm_rows(other, EPS)
    assert torch.equal(yo[3], y[37]) and torch.equal(ops.l2norm_rows_bwd(ocot, other, invo, EPS)[3], dx[37])
    # strided rows (a column slice of a wider tensor): same bits
    wide = _randn(g, 7, 2 * D, dtype=dtype)
    ys, _ = ops.l2norm_rows(wide[:, :D], EPS)
    assert torch.equal(ys, ops.l2norm_rows(wide[:, :D].contiguous(), EPS)[0])


def test_l2norm_refuses_what_the_kernel_does_not_take():
    from octic_vits_amd import ops
    x = torch.randn(4, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.l2norm_rows(x[:, :60])                                    # D % 8
    with pytest.raises(ValueError):
        ops.l2norm_rows(torch.randn(2, 4104, device="cuda"))          # D > 4096
    with pytest.raises(ValueError):
        ops.l2norm_rows(x.t())                                        # column stride
    with pytest.raises(TypeError):
        ops.l2norm_rows(x.half())
    y, inv = ops.l2norm_rows(x)
    with pytest.raises(ValueError):
        ops.l2norm_rows_bwd(x[:3], x, inv)
    with pytest.raises(ValueError):
        ops.l2norm_rows_bwd(x, x, inv[:3])


# --------------------------------------------------------------------------------------------------------- weight norm
WN_SHAPES = [(N, K) for N in (8, 72, 1000) for K in (64, 256)]


def _wn_case(N, K):
    g = _gen(N * 7 + K)
    v = _randn(g, N, K) * 0.02
    wg = 0.5 + torch.rand(N, 1, generator=g, device="cuda")           # not all ones
    return g, v, wg


def _bf16_ulp_of(t):
    """One bf16 ulp at every (bf16-representable) value of t."""
    _, e = torch.frexp(t.float().abs())
    return torch.ldexp(torch.ones_like(t, dtype=torch.float32), e - 1 - 7)


@pytest.mark.parametrize("N,K", WN_SHAPES)
def test_weight_norm_prep_operands(N, K):
    from octic_vits_amd import ops
    _, v, wg = _wn_case(N, K)
    w, wt, norms = ops.weight_norm_prep(v, wg)
    ref32 = torch._weight_norm(v, wg, 0)
    refb = ref32.to(torch.bfloat16)
    ours32 = wg * v * (1.0 / norms[:, None])                          # the header's arithmetic on the kernel's own norms
    same = ours32 == ref32
    print(f"f32 values agree on {float(same.float().mean()):.4f} of the elements")
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (N, K) and tuple(wt.shape) == (K, N)
    assert torch.equal(w[same], refb[same])
    assert bool(((w.float() - refb.float()).abs() <= _bf16_ulp_of(refb)).all())
    assert torch.equal(wt, w.t().contiguous())
    torch.testing.assert_close(norms.double(), v.double().norm(dim=1), rtol=2.0 ** -20, atol=0)
    # two calls: same bits; a row does not depend on the rows around it
    w2, wt2, norms2 = ops.weight_norm_prep(v, wg)
    assert torch.equal(w, w2) and torch.equal(wt, wt2) and torch.equal(norms, norms2)
    w8, _, n8 = ops.weight_norm_prep(v[N - 8:].clone(), wg[N - 8:].clone())
    assert torch.equal(w8, w[N - 8:]) and torch.equal(n8, norms[N - 8:])


@pytest.mark.parametrize("N,K", WN_SHAPES)
def test_weight_norm_prep_without_the_transposed_operand_writes_none(N, K):
    from octic_vits_amd import ops
    _, v, wg = _wn_case(N, K)
    w, _, norms = ops.weight_norm_prep(v, wg)
    planted = torch.full((K, N), -1.5, dtype=torch.bfloat16, device="cuda")
    w2, wt2, norms2 = ops.weight_norm_prep(v, wg, want_wt=False, wt_out=planted)
    assert wt2 is None and torch.equal(w2, w) and torch.equal(norms2, norms)
    assert bool((planted == -1.5).all())
    # ... and a caller's buffer is where W^T lands when it is asked for
    _, wt3, _ = ops.weight_norm_prep(v, wg, want_wt=True, wt_out=planted)
    assert wt3 is planted and torch.equal(planted, w.t().contiguous())


@pytest.mark.parametrize("N,K", WN_SHAPES)
def test_weight_norm_backward_against_float64(N, K):
    from octic_vits_amd import ops
    g, v, wg = _wn_case(N, K)
    dw = _randn(g, N, K)
    lv, lg = v.clone().requires_grad_(True), wg.clone().requires_grad_(True)
    torch._weight_norm(lv, lg, 0).backward(dw)
    v64, g64 = v.double().requires_grad_(True), wg.double().requires_grad_(True)
    torch._weight_norm(v64, g64, 0).backward(dw.double())
    _, _, norms = ops.weight_norm_prep(v, wg, want_wt=False)
    dv, dg = ops.weight_norm_bwd(dw, v, wg, norms)
    assert dv.dtype == dg.dtype == torch.float32 and dv.shape == v.shape and dg.shape == wg.shape
    _rule("dv", dv, lv.grad, v64.grad)
    _rule("dg", dg, lg.grad, g64.grad)
    dv2, dg2 = ops.weight_norm_bwd(dw, v, wg, norms)
    assert torch.equal(dv, dv2) and torch.equal(dg, dg2)


def test_weight_norm_refuses_what_the_kernels_do_not_take():
    from octic_vits_amd import ops
    v, wg = torch.randn(16, 64, device="cuda"), torch.ones(16, 1, device="cuda")
    with pytest.raises(ValueError):
        ops.weight_norm_prep(v[:, :60].contiguous(), wg)              # K % 8
    with pytest.raises(ValueError):
        ops.weight_norm_prep(v.bfloat16(), wg)
    with pytest.raises(ValueError):
        ops.weight_norm_prep(v, wg[:8])
    with pytest.raises(ValueError):
        ops.weight_norm_prep(v[:12].contiguous(), wg[:12].contiguous())          # W^T needs N % 8 == 0
    assert ops.weight_norm_prep(v[:12].contiguous(), wg[:12].contiguous(), want_wt=False)[1] is None
    _, _, norms = ops.weight_norm_prep(v, wg)
    with pytest.raises(ValueError):
        ops.weight_norm_bwd(v[:8], v, wg, norms)


# ----------------------------------------------------------------------------------------------------------- whole head
ISSUE_DIMS = (128, 128, 64, 264)       # in_dim, hidden, bottleneck, prototypes of the issue: outside ops.dense_gemm_ok (the GEMM
                                       # kernel needs K >= 128 and the routing N % 64 == 0), so this head keeps the stock path
ENGINE_DIMS = (128, 128, 128, 320)     # the smallest widths the engine path takes: one K pair of 64, a 64-column tail tile


def _make_head(dims, nlayers=3, seed=0, zero_bias=False):
    from octic_vits_amd import ssl as S
    in_dim, hidden, bottleneck, protos = dims
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        head = S.DINOHead(in_dim=in_dim, out_dim=protos, hidden_dim=hidden, bottleneck_dim=bottleneck, nlayers=nlayers)
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith("weight_g"):
                p.copy_(0.5 + torch.rand_like(p))
            elif n.endswith("bias"):
                p.zero_() if zero_bias else p.copy_(0.1 * torch.randn_like(p))
            else:
                p.copy_(torch.randn_like(p) / math.sqrt(p.shape[1]))
    return head.cuda()


def _clone_head(head, dims, nlayers, dtype=torch.float32):
    twin = _make_head(dims, nlayers, seed=1)
    twin.load_state_dict(head.state_dict())
    return twin.to(dtype)


def _run_head(head, x, cot, switch, autocast=True):
    """(output, input gradient, parameter gradients by name) of one forward + backward."""
    for p in head.parameters():
        p.grad = None
    leaf = x.clone().requires_grad_(True)
    with _switch(switch):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            y = head(leaf)
        y.backward(cot.to(y.dtype))
    return y.detach(), leaf.grad, {n: p.grad.clone() for n, p in head.named_parameters()}


def _check_head(dims, nlayers, rows, pad, zero_bias=False, seed=0):
    from octic_vits_amd import functional as OF
    head = _make_head(dims, nlayers, seed=seed, zero_bias=zero_bias)
    g = _gen(rows * 31 + nlayers)
    x = _randn(g, rows, dims[0])
    cot = _randn(g, rows, dims[3]) / dims[3]
    if pad:                                                           # the step's padding rows: +0 in, no cotangent back
        x[rows - pad:] = 0.0
        cot[rows - pad:] = 0.0
    with torch.autocast("cuda", dtype=torch.bfloat16):
        routed = OF.dino_head_ok(head, x)
    assert routed == (dims == ENGINE_DIMS or dims[0] == 1280)
    (y, dx, grads), names = _timed(lambda: _run_head(head, x, cot, True))
    ys, dxs, gs = _run_head(head, x, cot, False)
    ref = _clone_head(head, dims, nlayers, torch.float64)
    y64, dx64, g64 = _run_head(ref, x.double(), cot.double(), False, autocast=False)
    assert y.dtype == ys.dtype == torch.bfloat16 and dx.dtype == dxs.dtype and tuple(y.shape) == (rows, dims[3])
    assert any(n.startswith("weight_norm_prep_kernel") for n in names) == routed, names
    if routed:
        for k in ("weight_norm_prep_kernel<nt>", "weight_norm_bwd_kernel", "l2norm_fwd_kernel<bf16,bf16>",
                  "l2norm_bwd_kernel<bf16,bf16>", "dense_nt_kernel<prototypes>", "dense_nt_kernel<dprototypes>"):
            assert any(n.startswith(k) for n in names), (k, names)
        assert not any(n.startswith("library_gemm<fwd") or n.startswith("library_gemm<dgrad") for n in names), names
    _rule("out", y, ys, y64)
    _rule("dx", dx, dxs, dx64)
    assert set(grads) == set(gs) == set(g64)
    for n in sorted(grads):
        assert grads[n].dtype == torch.float32 and grads[n].shape == gs[n].shape
        _rule(n, grads[n], gs[n], g64[n])
    # the teacher's call: no_grad, same bits
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), _switch(True):
        (yt, tnames) = _timed(lambda: head(x))
    assert torch.equal(yt, y)
    if routed:
        assert any(n.startswith("weight_norm_prep_kernel<n>") for n in tnames), tnames
    return head


@pytest.mark.parametrize("rows,pad", [(1, 0), (40, 8), (257, 17)], ids=["1row", "40rows", "257rows"])
@pytest.mark.parametrize("nlayers", [1, 2, 3])
@pytest.mark.parametrize("dims", [ISSUE_DIMS, ENGINE_DIMS], ids=["128-128-64-264", "128-128-128-320"])
def test_small_head_against_float64(dims, nlayers, rows, pad):
    _check_head(dims, nlayers, rows, pad)


def test_small_head_with_zero_biases_and_zero_rows():
    """The state a fresh head is in: zero biases, so the padding rows are exactly zero through the whole MLP and meet the
    eps clamp of the normalisation - finite outputs and gradients, same rule."""
    _check_head(ENGINE_DIMS, 3, 40, 8, zero_bias=True)


def test_recipe_widths_once():
    """1280 -> 2048 -> 2048 -> 256 -> 65 536 at 40 rows, forward + backward."""
    _check_head((1280, 2048, 256, 65536), 3, 40, 8, seed=2)


# ------------------------------------------------------------------------------------------------------------ freshness
def _fresh_equals(head, dims, nlayers, x):
    """head(x) under autocast equals, bit for bit, a fresh head built from head's state dict."""
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), _switch(True):
        got = head(x)
        want = _clone_head(head, dims, nlayers)(x)
    assert torch.equal(got, want)
    return got


def test_next_call_uses_new_parameter_values():
    from octic_vits_amd import functional as OF
    head = _make_head(ENGINE_DIMS)
    x = _randn(_gen(3), 40, ENGINE_DIMS[0])
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert OF.dino_head_ok(head, x)
    y0 = _fresh_equals(head, ENGINE_DIMS, 3, x)
    head.load_state_dict(_make_head(ENGINE_DIMS, seed=5).state_dict())
    y1 = _fresh_equals(head, ENGINE_DIMS, 3, x)
    assert not torch.equal(y0, y1)
    with torch.no_grad():
        head.last_layer.weight_v.mul_(torch.linspace(0.5, 2.0, ENGINE_DIMS[2], device="cuda"))
    y2 = _fresh_equals(head, ENGINE_DIMS, 3, x)
    assert not torch.equal(y1, y2)
    with torch.no_grad():                                             # a raw write: no version counter moves
        head.mlp[0].weight.data.mul_(1.5)
        head.last_layer.weight_g.data.add_(0.25)
    assert not torch.equal(_fresh_equals(head, ENGINE_DIMS, 3, x), y2)
    OF.invalidate_weight_caches(head)                                 # nothing is cached: a no-op that must stay harmless
    _fresh_equals(head, ENGINE_DIMS, 3, x)


STEP_KW = dict(head_n_prototypes=256, head_hidden_dim=128, head_bottleneck_dim=128)
STEP_DIMS = (128, 128, 128, 256)


def _arch(seed=0, backbone=None, **kw):
    from octic_vits_amd import ssl as S
    from test_ssl_gpu import DIM, KW, _product_backbone
    torch.manual_seed(seed)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return S.SSLMetaArch(backbone or _product_backbone, DIM, koleo_loss_weight=0.1, **{**KW, **STEP_KW, **kw})


def _images(B, seed, dtype=torch.float32, device="cuda"):
    from octic_vits_amd import ssl as S
    random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    gc, lc = torch.randn(2 * B, 3, 32, 32, generator=g), torch.randn(2 * B, 3, 16, 16, generator=g)
    im = S.collate(gc, lc, (0.1, 0.5), 0.5, 64, S.MaskingGenerator((8, 8), max_num_patches=32))
    cast = lambda v: v.to(device, dtype) if v.is_floating_point() else v.to(device)
    return {k: (cast(v) if torch.is_tensor(v) else v) for k, v in im.items()}


@pytest.mark.parametrize("fused", [True, False], ids=["fused_step", "unfused_step"])
def test_heads_are_fresh_after_the_trainer_step_and_the_teacher_update(fused):
    from octic_vits_amd import ssl as S
    arch = _arch().cuda().train()
    tr = S.SSLTrainer(arch, lr=1e-3, fused_optimizer=fused)
    images = _images(4, 3)
    x = _randn(_gen(9), 24, STEP_DIMS[0])
    before = [_fresh_equals(arch.student["dino_head"], STEP_DIMS, 3, x), _fresh_equals(arch.teacher["dino_head"], STEP_DIMS, 3, x)]
    for _ in range(2):
        _, names = _timed(lambda: tr.step(images, teacher_temp=0.05, momentum=0.9))
        assert any(n.startswith("weight_norm_prep_kernel<nt>") for n in names), names      # the student's head
        assert any(n.startswith("weight_norm_prep_kernel<n>") for n in names), names       # the teacher's
        after = [_fresh_equals(arch.student["dino_head"], STEP_DIMS, 3, x), _fresh_equals(arch.teacher["dino_head"], STEP_DIMS, 3, x)]
        assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])
        before = after
    arch.update_teacher(0.5)
    assert not torch.equal(_fresh_equals(arch.teacher["dino_head"], STEP_DIMS, 3, x), before[1])


# -------------------------------------------------------------------------------------------------------------- routing
def _stock_composition(head, x):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        w = torch._weight_norm(head.last_layer.weight_v, head.last_layer.weight_g, 0)
        return F.linear(F.normalize(head.mlp(x), dim=-1, p=2, eps=EPS), w)


def test_dino_head_ok_refusals_on_the_device():
    """Every refusal of the predicate on CUDA tensors under bf16 autocast, where nothing but the refused property stands in the
    way: the same head and rows are accepted first."""
    from octic_vits_amd import functional as OF
    head = _make_head(ENGINE_DIMS)
    x = _randn(_gen(2), 40, ENGINE_DIMS[0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        from octic_vits_amd import ssl as S
        bn = S.DINOHead(in_dim=128, out_dim=320, hidden_dim=128, bottleneck_dim=128, use_bn=True).cuda()
    assert not OF.dino_head_ok(head, x)                                            # float32, no autocast
    with torch.autocast("cuda", dtype=torch.float16):
        assert not OF.dino_head_ok(head, x)                                        # fp16 autocast
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert OF.dino_head_ok(head, x) and OF.dino_head_ok(head, x.bfloat16())
        assert OF.dino_head_ok(_make_head(ENGINE_DIMS, nlayers=1), x) and OF.dino_head_ok(_make_head(ENGINE_DIMS, nlayers=2), x)
        assert not OF.dino_head_ok(bn, x)                                          # BatchNorm in the MLP
        assert not OF.dino_head_ok(head, x.cpu())                                  # CPU rows
        assert not OF.dino_head_ok(head, x.half())                                 # fp16 rows
        assert not OF.dino_head_ok(head, x[None])                                  # not [rows, in_dim]
        assert not OF.dino_head_ok(head, x[:0])                                    # no rows
        assert not OF.dino_head_ok(head, x[:, :64])                                # not the head's in_dim
        assert not OF.dino_head_ok(_make_head(ISSUE_DIMS), x)                      # bottleneck 64, 264 prototypes
        assert not OF.dino_head_ok(_make_head((128, 128, 128, 264)), x)            # prototypes % 64
        assert not OF.dino_head_ok(_make_head((128, 128, 64, 320)), x)             # K = 64 of the prototype GEMM
        assert not OF.dino_head_ok(_make_head((128, 96, 128, 320)), x)             # hidden width % 64
        assert not OF.dino_head_ok(_make_head(ENGINE_DIMS).double(), x)            # float64 parameters
        seen = []

        def probe(t):
            seen.append(OF.dino_head_ok(head, t))
            return t + 1

        torch.compile(probe, backend="eager")(x)                                   # tracing
        assert seen and not any(seen)
        assert OF.dino_head_ok(head, x)                                            # ... and accepted again outside the trace
    # a refused head under autocast runs the stock composition: no engine kernel
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16), _switch(True):
        y, names = _timed(lambda: bn.eval()(x))
    assert not any("weight_norm" in n or "l2norm" in n or "head-" in n for n in names), names


def test_switch_off_is_the_stock_module_bitwise():
    head = _make_head(ENGINE_DIMS)
    g = _gen(21)
    x, cot = _randn(g, 40, ENGINE_DIMS[0]), _randn(g, 40, ENGINE_DIMS[3])
    (y, dx, grads), names = _timed(lambda: _run_head(head, x, cot, False))
    assert not any("weight_norm" in n or "l2norm" in n or "head-" in n for n in names), names
    for p in head.parameters():
        p.grad = None
    leaf = x.clone().requires_grad_(True)
    want = _stock_composition(head, leaf)
    want.backward(cot.to(want.dtype))
    assert torch.equal(y, want.detach()) and torch.equal(dx, leaf.grad)
    for n, p in head.named_parameters():
        assert torch.equal(grads[n], p.grad), n
    # float32 without autocast keeps the stock composition whatever the switch says
    (y32, _, _), names32 = _timed(lambda: _run_head(head, x, cot, True, autocast=False))
    assert y32.dtype == torch.float32 and not any("weight_norm" in n or "l2norm" in n for n in names32), names32


_CHILD = """
import sys, warnings, torch
sys.path.insert(0, {tests!r})
warnings.simplefilter("ignore")
from octic_vits_amd import ssl as S, ops
from test_dino_head_engine_gpu import ENGINE_DIMS, _make_head, _timed
assert S.DINO_HEAD_HIP is {expect}
head = _make_head(ENGINE_DIMS)
x = torch.randn(40, ENGINE_DIMS[0], generator=torch.Generator(device="cuda").manual_seed(21), device="cuda")
with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    y, names = _timed(lambda: head(x))
torch.save({{"y": y.cpu(), "engine": any(n.startswith("weight_norm_prep_kernel") for n in names)}}, {out!r})
"""


def test_environment_switch_in_a_fresh_process(tmp_path):
    """OCTIC_DINO_HEAD_HIP=0 in a fresh child process: the stock module's results, bit for bit."""
    tests = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "child.pt")
    env = {**os.environ, "OCTIC_DINO_HEAD_HIP": "0"}
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(tests)] + [p for p in [env.get("PYTHONPATH")] if p])
    r = subprocess.run([sys.executable, "-c", _CHILD.format(tests=tests, expect="False", out=out)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    child = torch.load(out)
    assert child["engine"] is False
    head = _make_head(ENGINE_DIMS)
    x = torch.randn(40, ENGINE_DIMS[0], generator=_gen(21), device="cuda")
    with torch.no_grad():
        want = _stock_composition(head, x)
    assert torch.equal(child["y"], want.cpu())


# ------------------------------------------------------------------------------------------------------------- the step
def _three_steps(arch, images, switch, **trainer_kw):
    from octic_vits_amd import ssl as S
    with _switch(switch):
        tr = S.SSLTrainer(arch, lr=1e-3, **trainer_kw)
        losses = []
        for _ in range(3):
            out = tr.step(images, teacher_temp=0.05, momentum=0.9)
            losses.append({k: float(v.detach()) for k, v in out.items()})
    return losses, {n: p.detach().double().cpu() for n, p in arch.student.named_parameters()}


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _first_gradients(arch, images, switch, autocast):
    """Student gradients of ONE forward_backward on a fresh architecture: no clipping, no optimizer - deterministic."""
    with _switch(switch), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        arch.forward_backward(images, teacher_temp=0.05)
    return {n: p.grad.detach().double().cpu() for n, p in arch.student.named_parameters() if p.grad is not None}


def test_three_trainer_steps_switch_on_against_off():
    """SSLTrainer.step on the suite's tiny hybrid backbone, three iterations, the switch on against off, and both against the
    same three steps in float64 (the product architecture around the oracle's pure-torch backbone, on the CPU, same state
    dict).  The tolerance is the rule of this file with the off arm as the stock arm; the off arm's float64 errors are measured
    here and printed.
      * losses: per term and iteration |on - f64| <= 2 |off - f64| + 1 bf16 ulp of the term;
      * gradients of the first backward pass (no clipping, no optimizer: deterministic), PER TENSOR of the student, heads and
        backbone: max |on - f64| <= 2 max |off - f64| + 1 f32 ulp at the tensor's largest float64 gradient;
      * parameters after the three steps, per sub-model (backbone, dino_head): rms(on - f64) <= 2 rms(off - f64) + 1 f32 ulp.
        AdamW's first update of an element is lr sign(g), so an element whose gradient sign lies inside the bf16 noise moves by
        a multiple of lr in either arm and WHICH elements those are is chance: a tensor's max error is 0 or about 2 lr by luck
        (taken tensor by tensor in the max norm this rule failed on 5 of 159 tensors, e.g. 2.0e-3 against 1.3e-4, with a head
        that passes every gradient check), while the root mean square over a sub-model's tens of thousands of elements measures
        how MANY elements went astray: a wrong gradient of one head tensor (say the sign of dv) moves all of its elements the
        wrong way, 2 lr per step, and multiplies the head's rms several times over.
    Two runs with the switch on are bitwise equal."""
    from test_ssl_gpu import _oracle_backbone
    state = None

    def fresh(backbone=None):
        nonlocal state
        arch = _arch(backbone=backbone)
        if state is None:
            state = {k: v.clone() for k, v in arch.state_dict().items()}
        arch.load_state_dict(state)
        return arch

    def run(switch):
        torch.manual_seed(123)
        return _three_steps(fresh().cuda().train(), _images(4, 3), switch)

    bad = []
    # ---- gradients of the first backward pass
    g_on = _first_gradients(fresh().cuda().train(), _images(4, 3), True, True)
    g_off = _first_gradients(fresh().cuda().train(), _images(4, 3), False, True)
    g_ref = _first_gradients(fresh(_oracle_backbone).double().train(), _images(4, 3, torch.float64, "cpu"), False, False)
    assert set(g_on) == set(g_off) == set(g_ref) and len(g_ref) > 60
    assert all(n in g_ref for n in ("dino_head.last_layer.weight_v", "dino_head.last_layer.weight_g", "dino_head.mlp.0.weight"))
    for n in sorted(g_ref):
        e_on, e_off = float((g_on[n] - g_ref[n]).abs().max()), float((g_off[n] - g_ref[n]).abs().max())
        bound = 2.0 * e_off + _ulp(torch.float32, float(g_ref[n].abs().max()))
        print(f"gradient {n}: max|f64| {float(g_ref[n].abs().max()):.3e}  off err {e_off:.3e}  on err {e_on:.3e}  bound {bound:.3e}")
        if not (bool(torch.isfinite(g_on[n]).all()) and e_on <= bound):
            bad.append(("gradient", n, e_on, e_off, bound))
    # ---- three steps
    (on, p_on), names = _timed(lambda: run(True))
    assert any(n.startswith("weight_norm_bwd_kernel") for n in names), names
    on2, p_on2 = run(True)
    off, p_off = run(False)
    assert on == on2 and all(torch.equal(p_on[n], p_on2[n]) for n in p_on)
    ref, p_ref = _three_steps(fresh(_oracle_backbone).double().train(), _images(4, 3, torch.float64, "cpu"), False, autocast=False,
                              fused_optimizer=False)
    for it in range(3):
        for k in ref[it]:
            e_on, e_off = abs(on[it][k] - ref[it][k]), abs(off[it][k] - ref[it][k])
            bound = 2.0 * e_off + _ulp(torch.bfloat16, abs(ref[it][k]))
            print(f"iteration {it} {k}: f64 {ref[it][k]:.6f}  off err {e_off:.3e}  on err {e_on:.3e}  bound {bound:.3e}")
            if not (math.isfinite(on[it][k]) and e_on <= bound):
                bad.append((it, k, e_on, bound))
    assert set(p_on) == set(p_off) == set(p_ref)
    assert all(bool(torch.isfinite(p_on[n]).all()) for n in p_on)
    subs = sorted({n.split(".")[0] for n in p_ref})
    assert "dino_head" in subs and "backbone" in subs
    for sub in subs:
        names_ = [n for n in sorted(p_ref) if n.split(".")[0] == sub]
        cat = lambda p: torch.cat([(p[n] - p_ref[n]).flatten() for n in names_])
        r_on, r_off = _rms(cat(p_on)), _rms(cat(p_off))
        top = max(float(p_ref[n].abs().max()) for n in names_)
        bound = 2.0 * r_off + _ulp(torch.float32, top)
        print(f"parameters of {sub} after 3 steps ({sum(p_ref[n].numel() for n in names_)} elements): rms off err {r_off:.3e}  "
              f"rms on err {r_on:.3e}  bound {bound:.3e}")
        if not r_on <= bound:
            bad.append(("parameters", sub, r_on, r_off, bound))
    assert not bad, bad
