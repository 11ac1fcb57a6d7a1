"""The float32 dense GEMM family (csrc/dense_f32.hip) on the MI355X: exact operands against float64 bitwise at every tile, K-block
and slab edge, random operands inside the measured error of the f32 MFMA chain, the GELU epilogue and backward against ATen's
own error, independence of batch mates, sentinels around every output and workspace, repeatability and graph capture, the
autograd functions, a float32 block stack without library GEMMs, and parity with the reference goldens and the stock path.

Tolerance of the random-operand checks: |y - y64| <= 4e-7 * (sum_k |a||w| + |bias|) per element (the measured error of this
MFMA chain, 3.5e-7 * sum at K = 4096, scaled by sqrt(K) to the longest reduction used here, 5120)."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import baseline_cases as BC
from octic_vits_amd import _lib, functional as OF, ops

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NT, NN, TN = _lib.DENSE_F32_NT, _lib.DENSE_F32_NN, _lib.DENSE_F32_TN
C = 4e-7
DEV = "cuda"


def _ints(seed, *shape, ld=None):
    """Integer-valued float32 in [-8, 8]; ld: row stride of the returned 2-D view (a slice of a wider buffer full of 99)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-8, 9, shape, generator=g).float().to(DEV)
    return _strided(t, ld)


def _rand(seed, *shape, ld=None):
    g = torch.Generator().manual_seed(seed)
    return _strided(torch.randn(shape, generator=g).to(DEV), ld)


def _strided(t, ld):
    if ld is None:
        return t
    buf = torch.full((t.shape[0], ld), 99.0, device=DEV)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def _mm64(a, b):
    return a.double() @ b.double()


def _run(op, M, N, K, pad=0, bias=True, seed=0, make=_ints):
    """One product on operands from `make` with row strides length + pad -> (result tensors, float64 expectations)."""
    ld = (lambda n: n + pad) if pad else (lambda n: None)
    if op == NT:
        a, w = make(seed, M, K, ld=ld(K)), make(seed + 1, N, K, ld=ld(K))
        b = make(seed + 2, N) if bias else None
        want = _mm64(a, w.t()) + (b.double() if bias else 0)
        return (ops.dense_f32_nt(a, w, b),), (want,)
    if op == NN:
        g, w = make(seed, M, N, ld=ld(N)), make(seed + 1, N, K, ld=ld(K))
        return (ops.dense_f32_nn(g, w),), (_mm64(g, w),)
    g, x = make(seed, M, N, ld=ld(N)), make(seed + 1, M, K, ld=ld(K))
    dw, db = ops.dense_f32_tn(g, x, want_colsum=True)
    return (dw, db), (_mm64(g.t(), x), g.double().sum(0))


def _assert_exact(got, want, what):
    for y, y64 in zip(got, want):
        assert y.dtype == torch.float32 and y.shape == y64.shape, what
        assert torch.equal(y.double(), y64), f"{what}: {int((y.double() != y64).sum())} of {y.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ 1. exact operands
_MS = (1, 15, 16, 17, 127, 128, 129, 257, 514)
_NS = (4, 12, 16, 20, 124, 128, 132, 260)
_KS = (4, 8, 28, 32, 36, 64, 68, 132)
_SPARSE = sorted({(_MS[i], _NS[i % 8], _KS[(3 * i) % 8]) for i in range(9)}
                 | {(_MS[(2 * i + 1) % 9], _NS[(5 * i + 2) % 8], _KS[i]) for i in range(8)}
                 | {(_MS[(4 * i) % 9], _NS[i], _KS[(7 * i + 5) % 8]) for i in range(8)})


def test_the_sparse_cross_covers_every_listed_size():
    assert {m for m, _, _ in _SPARSE} == set(_MS) and {n for _, n, _ in _SPARSE} == set(_NS) and {k for _, _, k in _SPARSE} == set(_KS)


@pytest.mark.parametrize("op", [NT, NN, TN])
@pytest.mark.parametrize("M,N,K", _SPARSE)
def test_integer_operands_equal_float64_bitwise(op, M, N, K):
    got, want = _run(op, M, N, K, seed=M + N + K)
    _assert_exact(got, want, f"op {op} {M}x{N}x{K}")
    if op == NT:
        got, want = _run(op, M, N, K, bias=False, seed=M + N + K)
        _assert_exact(got, want, f"NT without bias {M}x{N}x{K}")


def _plan_edges():
    """One case on each side of every output-tile edge and every TN slab edge octic_dense_f32_plan reports (the K-block edges
    are the K = 28 / 32 / 36 and 64 / 68 of the sparse cross: the plan's four numbers do not name the K block)."""
    if not os.path.exists(_lib.LIB_PATH):              # (collection asks the library: a fresh checkout builds it first)
        from octic_vits_amd.build import build
        build()
    cases = []
    for op in (NT, NN, TN):
        tr, tc, _, _ = ops.dense_f32_plan(op, 64, 64, 64)
        for rows in (tr - 1, tr, tr + 1, 2 * tr + 1):
            for cols in (tc - 4, tc, tc + 4):
                # output rows / columns are (M, N) for NT, (M, K) for NN and (N, K) for TN
                r4 = -(-rows // 4) * 4 if op == TN else rows
                cases.append({NT: (op, r4, cols, 36), NN: (op, r4, 36, cols), TN: (op, 37, r4, cols)}[op])
        assert ops.dense_f32_plan(op, tr, tc, tc)[3] == 1 and ops.dense_f32_plan(op, tr + 4, tc + 4, tc + 4)[3] > 1
    slabs = [ops.dense_f32_plan(TN, M, 16, 20)[2] for M in range(1, 1400)]
    edges = [M for M in range(2, 1400) if slabs[M - 1] != slabs[M - 2]]
    assert edges and max(slabs) >= 4, "the TN plan never splits these rows: pick a wider scan"
    for M in edges:
        cases += [(TN, M - 1, 16, 20), (TN, M, 16, 20), (TN, M + 1, 16, 20)]
    return sorted(set(cases))


@pytest.mark.parametrize("op,M,N,K", _plan_edges())
def test_integer_operands_at_the_plans_tile_and_slab_edges(op, M, N, K):
    _assert_exact(*_run(op, M, N, K, seed=7 * M + N + K), f"op {op} {M}x{N}x{K}")


@pytest.mark.parametrize("op", [NT, NN, TN])
@pytest.mark.parametrize("M,N,K,pad", [(17, 20, 36, 4), (129, 132, 68, 12), (514, 16, 28, 64)])
def test_integer_operands_with_row_strides_beyond_the_row_length(op, M, N, K, pad):
    _assert_exact(*_run(op, M, N, K, pad=pad, seed=M), f"op {op} {M}x{N}x{K} pad {pad}")


@pytest.mark.parametrize("N,K", [(3840, 1280), (1280, 5120)])
def test_integer_operands_model_shaped(N, K):
    for op in (NT, NN, TN):
        _assert_exact(*_run(op, 2 * 257, N, K, seed=N), f"op {op} 514x{N}x{K}")


# ------------------------------------------------------------------------------------------------ 2. random operands
def _bound(a_abs, b_abs, bias=None):
    s = a_abs.double() @ b_abs.double()
    return C * (s + (bias.double().abs() if bias is not None else 0))


@pytest.mark.parametrize("M,N,K", [(64, 128, 5120), (17, 132, 68), (257, 260, 1280), (1, 4, 4)])
def test_nt_and_nn_random_operands_within_the_mfma_chain_error(M, N, K):
    a, w, b = _rand(1, M, K), _rand(2, N, K), _rand(3, N)
    y = ops.dense_f32_nt(a, w, b)
    err, tol = (y.double() - (_mm64(a, w.t()) + b.double())).abs(), _bound(a.abs(), w.abs().t(), b)
    print(f"NT {M}x{N}x{K}: max err / (sum|a||w| + |b|) = {float((err / tol).max()) * C:.3e}")
    assert bool((err <= tol).all())
    # NN reduces over N: the layer turned round keeps the reduction at 5120 at most
    g = _rand(4, M, K)
    wt = _rand(5, K, N)
    dx = ops.dense_f32_nn(g, wt)
    err, tol = (dx.double() - _mm64(g, wt)).abs(), _bound(g.abs(), wt.abs())
    print(f"NN {M}x{K}x{N}: max err / sum|g||w| = {float((err / tol).max()) * C:.3e}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("M,N,K", [(5120, 20, 36), (514, 132, 260), (1285, 16, 16), (1, 4, 4)])
def test_tn_random_operands_within_the_mfma_chain_error(M, N, K):
    g, x = _rand(6, M, N), _rand(7, M, K)
    dw, db = ops.dense_f32_tn(g, x, want_colsum=True)
    err, tol = (dw.double() - _mm64(g.t(), x)).abs(), _bound(g.abs().t(), x.abs())
    print(f"TN {M}x{N}x{K} ({ops.dense_f32_plan(TN, M, N, K)[2]} slabs): max err / sum|g||x| = {float((err / tol).max()) * C:.3e}")
    assert bool((err <= tol).all())
    assert bool(((db.double() - g.double().sum(0)).abs() <= C * g.double().abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ 3. GELU
def _gelu64(h):
    return F.gelu(h.double())


@pytest.mark.parametrize("M,N,K", [(257, 260, 68), (64, 1536, 384)])
def test_gelu_epilogue_and_backward_against_atens_own_error(M, N, K):
    a, w, b = _rand(11, M, K), _rand(12, N, K), _rand(13, N)
    a[0, :] *= 6.0                                     # a row of large pre-activations: both tails of erf
    h, c = ops.dense_f32_nt(a, w, b, gelu=True)
    assert bool(((h.double() - (_mm64(a, w.t()) + b.double())).abs() <= _bound(a.abs(), w.abs().t(), b)).all())
    assert torch.equal(h, ops.dense_f32_nt(a, w, b))   # the pre-activation is the plain product
    want = _gelu64(h)
    ours, aten = float((c.double() - want).abs().max()), float((F.gelu(h).double() - want).abs().max())
    print(f"gelu epilogue {M}x{N}x{K}: max |err| kernel {ours:.3e}, ATen f32 {aten:.3e}")
    assert ours <= 2 * aten
    g = _rand(14, M, N)
    dh, db = ops.dense_gelu_bwd_f32(h, g)
    h64 = h.double().requires_grad_(True)
    want, = torch.autograd.grad(F.gelu(h64), h64, g.double())
    h32 = h.clone().requires_grad_(True)
    ref, = torch.autograd.grad(F.gelu(h32), h32, g)
    ours, aten = float((dh.double() - want).abs().max()), float((ref.double() - want).abs().max())
    print(f"gelu backward {M}x{N}: max |err| kernel {ours:.3e}, ATen f32 {aten:.3e}")
    assert ours <= 2 * aten
    # the bias gradient: column sums of the kernel's own dh (256 row blocks, fixed order)
    assert bool(((db.double() - dh.double().sum(0)).abs() <= C * dh.double().abs().sum(0)).all())
    dh2, none = ops.dense_gelu_bwd_f32(h, g, want_colsum=False)
    assert none is None and torch.equal(dh2, dh)


def test_gelu_backward_integer_column_sums_are_exact():
    h = torch.zeros(1031, 20, device=DEV)                # gelu'(0) = 0.5: dh = g / 2, every partial sum exact
    g = 2 * _ints(3, 1031, 20)
    dh, db = ops.dense_gelu_bwd_f32(h, g)
    assert torch.equal(dh, g / 2) and torch.equal(db.double(), (g / 2).double().sum(0))


# ------------------------------------------------------------------------------------------------ 4. batch mates
def test_rows_do_not_depend_on_their_batch_mates():
    N, K = 132, 260
    w, b = _rand(21, N, K), _rand(22, N)
    rows = _rand(23, 3, K)
    grows = _rand(24, 3, N)
    for r in range(3):
        alone = ops.dense_f32_nt(rows[r:r + 1], w, b)
        galone = ops.dense_f32_nn(grows[r:r + 1], w)
        for M, at in ((17, 5 + r), (300, 297 + r)):
            a, g = _rand(25 + M, M, K), _rand(26 + M, M, N)
            a[at], g[at] = rows[r], grows[r]
            assert torch.equal(ops.dense_f32_nt(a, w, b)[at:at + 1], alone)
            assert torch.equal(ops.dense_f32_nn(g, w)[at:at + 1], galone)
            # ... nor on the strides: the same data as a view of wider rows
            assert torch.equal(ops.dense_f32_nt(_strided(a, K + 12), _strided(w, K + 4), b)[at:at + 1], alone)
            assert torch.equal(ops.dense_f32_nn(_strided(g, N + 8), _strided(w, K + 4))[at:at + 1], galone)
        h, c = ops.dense_f32_nt(rows[r:r + 1], w, b, gelu=True)
        a = _rand(40, 129, K)
        a[128] = rows[r]
        h2, c2 = ops.dense_f32_nt(a, w, b, gelu=True)
        assert torch.equal(h2[128:], h) and torch.equal(c2[128:], c) and torch.equal(h, alone)


# ------------------------------------------------------------------------------------------------ 5. edges
SENT = -12345.0


def _framed(rows, cols, ld, guard=3):
    """A [rows, cols] view (row stride ld) in the middle of a buffer full of SENT -> (view, check()) with check asserting that
    nothing but the view's elements changed."""
    buf = torch.full((rows + 2 * guard, ld), SENT, device=DEV)
    view = buf[guard:guard + rows, :cols]

    def check():
        probe = buf.clone()
        probe[guard:guard + rows, :cols] = SENT
        assert bool((probe == SENT).all()), "a launch wrote outside its output"
        assert bool((view != SENT).all()), "a launch left part of its output unwritten"
    return view, check


def _at_end(t):
    """The same values in the last bytes of a fresh allocation (behind a 16-byte aligned offset)."""
    flat = torch.empty(t.numel() + 52, device=DEV)
    flat[52:] = t.reshape(-1)
    return flat[52:].view(t.shape)


@pytest.mark.parametrize("M,N,K", [(129, 132, 36), (17, 20, 68), (128, 128, 32), (257, 4, 4)])
def test_nothing_outside_the_outputs_and_the_workspace_is_written(M, N, K):
    a, w, b, g = _at_end(_ints(1, M, K)), _at_end(_ints(2, N, K)), _at_end(_ints(3, N)), _at_end(_ints(4, M, N))
    out, ok = _framed(M, N, N + 8)
    ops.dense_f32_nt(a, w, b, out=out)
    ok()
    assert torch.equal(out.double(), _mm64(a, w.t()) + b.double())
    out, ok = _framed(M, N, N + 4)
    hout, hok = _framed(M, N, N + 12)
    ops.dense_f32_nt(a, w, b, gelu=True, out=out, h_out=hout)
    ok(), hok()
    assert torch.equal(hout.double(), _mm64(a, w.t()) + b.double())
    out, ok = _framed(M, K, K + 8)
    ops.dense_f32_nn(g, w, out=out)
    ok()
    assert torch.equal(out.double(), _mm64(g, w))
    for rows in (M, 514 + M):                           # one slab, several slabs
        g2, x2 = _at_end(_ints(5, rows, N)), _at_end(_ints(6, rows, K))
        need = int(_lib.lib().octic_dense_f32_workspace_bytes(TN, rows, N, K))
        wsbuf = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
        out, ok = _framed(N, K, K + 8)
        dw, db = ops.dense_f32_tn(g2, x2, out=out, want_colsum=True, workspace=wsbuf[256:256 + need])
        ok()
        assert dw is out and torch.equal(out.double(), _mm64(g2.t(), x2)) and torch.equal(db.double(), g2.double().sum(0))
        assert bool((wsbuf[:256] == 0x5A).all()) and bool((wsbuf[256 + need:] == 0x5A).all())
    h, gg = _at_end(_rand(7, M, N)), _at_end(_rand(8, M, N))
    dh, db = ops.dense_gelu_bwd_f32(h, gg)
    assert bool(torch.isfinite(dh).all()) and bool(torch.isfinite(db).all())


# ------------------------------------------------------------------------------------------------ 6. repeatability, capture
def _chain(a, w, b, g):
    h, c = ops.dense_f32_nt(a, w, b, gelu=True)
    dh, db = ops.dense_gelu_bwd_f32(h, g)
    dx = ops.dense_f32_nn(dh, w)
    dw, db2 = ops.dense_f32_tn(dh, a, want_colsum=True)
    return h, c, dh, db, dx, dw, db2


def test_two_launches_are_bitwise_equal_and_a_captured_graph_equals_eager():
    M, N, K = 1285, 260, 132                            # several TN slabs
    assert ops.dense_f32_plan(TN, M, N, K)[2] > 1
    a, w, b, g = _rand(31, M, K), _rand(32, N, K), _rand(33, N), _rand(34, M, N)
    first = _chain(a, w, b, g)
    for x, y in zip(first, _chain(a, w, b, g)):
        assert torch.equal(x, y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(a, w, b, g)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _chain(a, w, b, g)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(first, captured):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 7. autograd
@pytest.mark.parametrize("gelu", [False, True])
def test_autograd_functions_match_float64(gelu):
    B, T, K, N = 2, 129, 68, 132
    x = _rand(41, B, T, K).requires_grad_(True)
    lin = nn.Linear(K, N).to(DEV)
    gy = _rand(42, B, T, N)
    cache = OF.DenseWeightCache()
    if gelu:
        y = OF.DenseLinearGeluFn.apply(x, lin.weight, lin.bias, cache, torch.float32)
    else:
        y = OF.DenseLinearFn.apply(x, lin.weight, lin.bias, torch.float32, cache)
    gx, gw, gb = torch.autograd.grad(y, [x, lin.weight, lin.bias], gy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (x, lin.weight, lin.bias))
    h64 = F.linear(x64, w64, b64)
    y64 = F.gelu(h64) if gelu else h64
    gx64, gw64, gb64 = torch.autograd.grad(y64, [x64, w64, b64], gy.double())
    x2, g2 = x64.detach().reshape(-1, K), gy.double().reshape(-1, N)
    dh_tol = C * (x2.abs() @ w64.detach().abs().t() + b64.detach().abs())            # the GEMM's own bound on h
    if gelu:
        # |gelu'| <= 1.13 and |gelu''| <= 0.8: y inherits 1.13 x the error of h plus a few roundings of its own; the cotangent
        # dh = gelu'(h) gy inherits 0.8 |gy| x the error of h plus a few roundings, and the three gradients carry that on top of
        # their own GEMM bounds
        eps = 2.0 ** -23
        y_tol = 1.13 * dh_tol + 4 * eps * y64.detach().abs().reshape(-1, N) + 1e-30
        dh64 = torch.autograd.grad(F.gelu(h64), h64, gy.double())[0].reshape(-1, N)
        ddh = g2.abs() * (0.8 * dh_tol + 8 * eps)
    else:
        y_tol, dh64, ddh = dh_tol, g2, torch.zeros_like(g2)
    assert bool(((y.double().reshape(-1, N) - y64.detach().reshape(-1, N)).abs() <= y_tol).all())
    w_abs = w64.detach().abs()
    assert bool(((gx.double().reshape(-1, K) - gx64.reshape(-1, K)).abs() <= C * (dh64.abs() @ w_abs) + ddh @ w_abs).all())
    assert bool(((gw.double() - gw64).abs() <= C * (dh64.abs().t() @ x2.abs()) + ddh.t() @ x2.abs()).all())
    assert bool(((gb.double() - gb64).abs() <= C * dh64.abs().sum(0) + ddh.sum(0)).all())


def test_weight_gradient_lands_in_a_given_grad_dest_view(monkeypatch):
    K, N = 68, 132
    lin = nn.Linear(K, N).to(DEV)
    bucket = torch.full((N * K + 64,), SENT, device=DEV)
    view = bucket[32:32 + N * K].view(N, K)
    monkeypatch.setattr(ops, "GRAD_DEST", {lin.weight.data_ptr(): view})
    x, gy = _rand(43, 300, K), _rand(44, 300, N)
    y = OF.DenseLinearFn.apply(x, lin.weight, lin.bias, torch.float32, OF.DenseWeightCache())
    y.backward(gy)
    assert torch.equal(view, ops.dense_f32_tn(gy, x)) and torch.equal(lin.weight.grad, view)
    assert bool((bucket[:32] == SENT).all()) and bool((bucket[32 + N * K:] == SENT).all())


# ------------------------------------------------------------------------------------------------ 8. blocks
_FORBIDDEN_ATEN = ("mm", "addmm", "bmm", "baddbmm", "matmul", "linear", "native_layer_norm", "native_layer_norm_backward",
                   "gelu", "gelu_backward")
LS = ["deit_tiny_patch16_LS", "deit_small_patch16_LS", "deit_medium_patch16_LS", "deit_base_patch16_LS",
      "deit_large_patch16_LS", "deit_huge_patch14_LS"]


class _DispatchLog(torch.utils._python_dispatch.TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = set()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.add(func.overloadpacket.__name__)
        return func(*args, **(kwargs or {}))


def _deit_stack(name):
    from octic_vits_amd.deit_models import create_model
    torch.manual_seed(1)
    net = create_model(name, num_classes=10, drop_path_rate=0.1)
    net.blocks = nn.ModuleList(net.blocks[:2])                    # the factory's dims at a reduced depth
    del net.blocks[-1]._next_norm
    net = net.to(DEV).train()
    x = torch.randn(2, 3, 224, 224, device=DEV)
    return net.blocks, net.patch_embed.tokens(x, net.pos_embed[0], net.cls_token.flatten()).detach()


def _dino_swiglu_stack(_name):
    from octic_vits_amd.vit import NestedTensorBlock, SwiGLUFFNFused
    torch.manual_seed(2)
    blocks = nn.ModuleList([NestedTensorBlock(384, 6, mlp_ratio=4.0, qkv_bias=True, init_values=1e-5, ffn_layer=SwiGLUFFNFused)
                            for _ in range(2)]).to(DEV).train()
    return blocks, torch.randn(2, 257, 384, device=DEV)


def _run_stack(blocks, tok, monkeypatch, strict):
    """Forward + backward in float32 without autocast; the library entry points are patched to record (and, when strict,
    raise).  -> (python entry points reached, ATen ops dispatched)."""
    reached = []

    def trap(name, real):
        def f(*a, **k):
            reached.append(name)
            if strict:
                raise AssertionError(f"{name}: a library / ATen path was reached inside the float32 block stack")
            return real(*a, **k)
        return f
    cot = torch.randn_like(tok)
    log = _DispatchLog()
    with monkeypatch.context() as m:
        for mod, attr in ((F, "linear"), (torch, "mm"), (torch, "bmm"), (torch, "matmul"), (torch, "addmm"), (F, "layer_norm"),
                          (F, "gelu"), (F, "scaled_dot_product_attention")):
            m.setattr(mod, attr, trap(attr, getattr(mod, attr)))
        with log:
            t = tok
            for blk in blocks:
                t = blk(t)
            assert t.dtype == torch.float32
            (t * cot).sum().backward()
    torch.cuda.synchronize()
    return reached, log.seen


@pytest.mark.parametrize("name,make", [(n, _deit_stack) for n in LS] + [("dinov2_swiglu", _dino_swiglu_stack)])
def test_float32_block_stack_stays_on_hip(name, make, monkeypatch):
    blocks, tok = make(name)
    assert OF.DENSE_F32_HIP is True and not torch.is_autocast_enabled("cuda")
    reached, seen = _run_stack(blocks, tok, monkeypatch, strict=True)
    bad = {op for op in seen if op in _FORBIDDEN_ATEN or "scaled_dot_product" in op or "flash_attention" in op
           or "efficient_attention" in op}
    assert not reached and not bad, (reached, sorted(bad))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in blocks.parameters())
    # the control: with the switch off the same run is the stock composition
    for p in blocks.parameters():
        p.grad = None
    monkeypatch.setattr(OF, "DENSE_F32_HIP", False)
    reached, seen = _run_stack(blocks, tok, monkeypatch, strict=False)
    assert "linear" in reached and (set(_FORBIDDEN_ATEN) & seen)


def test_float32_regime_starts_at_head_dim_32(monkeypatch):
    """vit.F32_MIN_HEAD_DIM: a float32 block with head_dim 16 is the stock composition (the call site that
    tests/test_dense_gpu.py pins there), the same block with head_dim 32 runs on the kernels."""
    from octic_vits_amd import vit
    assert vit.F32_MIN_HEAD_DIM == 32
    for heads, engine in ((4, False), (2, True)):
        torch.manual_seed(3)
        blocks = nn.ModuleList([vit.Layer_scale_init_Block(64, heads, qkv_bias=True, init_values=0.5)]).to(DEV).train()
        reached, seen = _run_stack(blocks, torch.randn(2, 10, 64, device=DEV), monkeypatch, strict=False)
        assert ("linear" in reached) == (not engine) and bool(set(_FORBIDDEN_ATEN) & seen) == (not engine), (heads, reached)
        assert all(p.grad is not None for p in blocks.parameters())


# ------------------------------------------------------------------------------------------------ 9. parity
def _check_golden(name, got, tol=1e-3):
    want = np.load(os.path.join(GOLDEN, name + ".npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        if not want[k].size:
            continue
        scale = max(1.0, float(np.abs(want[k]).max()))
        err = float(np.abs(got[k] - want[k]).max())
        assert err <= tol * scale, f"{name}:{k} max err {err:.3e} scale {scale:.3g}"


def _count_calls(monkeypatch, name):
    real, calls = getattr(ops, name), []
    monkeypatch.setattr(ops, name, lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_float32_goldens_through_the_new_path(monkeypatch):
    from functools import partial
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    from octic_vits_amd.vit_models import vit_models
    calls = _count_calls(monkeypatch, "dense_f32_nt")
    make = lambda **kw: vit_models(mlp_ratio=4, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), **kw)
    _check_golden("baseline_deit_p16", BC.run_deit_case(make, "baseline_deit_p16", device=DEV))
    n_deit = len(calls)
    _check_golden("baseline_dino", BC.run_dino_case(lambda **kw: DinoVisionTransformer(**kw), "baseline_dino", device=DEV))
    assert n_deit >= 8 and len(calls) > n_deit            # four GEMMs per block, two blocks, on the float32 kernels


def test_float32_block_engine_against_stock_against_float64(monkeypatch):
    """Forward and parameter gradients of one float32 block, engine (switch on) and stock (switch off), both against a float64
    CPU run of the same module: the engine's max error may be 8 x the stock path's (a k-ordered chain at K = 5120 measured
    about 4 x less accurate than blocked summation, times 2)."""
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(5)
    blk = Layer_scale_init_Block(384, 6, mlp_ratio=4.0, qkv_bias=True, init_values=1.0).to(DEV).train()
    x = torch.randn(2, 197, 384, device=DEV)
    cot = torch.randn_like(x)
    ref = copy.deepcopy(blk).double().cpu()
    x64 = x.double().cpu().requires_grad_(True)
    y64 = ref(x64)
    g64 = torch.autograd.grad(y64, [x64] + list(ref.parameters()), cot.double().cpu())

    def run(on):
        monkeypatch.setattr(OF, "DENSE_F32_HIP", on)
        xx = x.clone().requires_grad_(True)
        y = blk(xx)
        g = torch.autograd.grad(y, [xx] + list(blk.parameters()), cot)
        fwd = float((y.detach().double().cpu() - y64.detach()).abs().max() / y64.detach().abs().max())
        bwd = max(float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g, g64))
        return fwd, bwd
    calls = _count_calls(monkeypatch, "dense_f32_tn")
    eng, n_on = run(True), len(calls)
    stock = run(False)
    assert n_on == 4 and len(calls) == 4                   # the four weight gradients ran on the kernels, then on the library
    print(f"float32 block, max rel err against float64: engine fwd {eng[0]:.3e} bwd {eng[1]:.3e}; stock fwd {stock[0]:.3e} "
          f"bwd {stock[1]:.3e}; ratios {eng[0] / stock[0]:.2f} / {eng[1] / stock[1]:.2f}")
    assert eng[0] <= 8 * stock[0] and eng[1] <= 8 * stock[1]
