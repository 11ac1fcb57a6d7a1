"""The DINO / iBOT head on the engine (csrc/dino_norm.hip, functional.dino_head_forward, ssl.DINO_HEAD_HIP), the part that needs
no GPU: why a backward pass through a DINOHead must never be captured in a hipGraph or run on a side stream, the argument
checks of the new entry points through the C ABI, the routing predicate's refusals, the state-dict keys, and the three kernels'
formulas restated in float64 against autograd of F.normalize and torch._weight_norm."""
import ctypes
import warnings

import pytest
import torch
import torch.nn.functional as F

from octic_vits_amd import _lib


def _head(**kw):
    from octic_vits_amd import ssl as S
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        args = dict(in_dim=128, out_dim=320, hidden_dim=128, bottleneck_dim=128)
        args.update(kw)
        return S.DINOHead(**args)


def _accumulate_grad_nodes(fn):
    """Every AccumulateGrad node reachable from an autograd node."""
    seen, found, todo = set(), [], [fn]
    while todo:
        n = todo.pop()
        if n is None or id(n) in seen:
            continue
        seen.add(id(n))
        if type(n).__name__ == "AccumulateGrad":
            found.append(n)
        todo.extend(m for m, _ in n.next_functions)
    return found


def test_stock_head_keeps_its_accumulate_grad_nodes_for_good():
    """nn.utils.weight_norm leaves last_layer.weight on the module: a non-leaf tensor whose graph holds the AccumulateGrad nodes
    of weight_g and weight_v, and every forward pre-hook builds the next one from the same parameters before the old one goes.
    The nodes are therefore the same OBJECTS after the constructor, after a forward + backward with every output deleted, and
    after the next forward - stamped for good with the stream the head was built on.  A graph capture runs on a side stream, so
    a captured backward through this module makes the autograd engine synchronise the capturing stream with the default one,
    the case torch's own warning names ("may ... break CUDA graph capture if the AccumulateGrad node's stream is the default
    stream").  Hence: eager only, default stream only (NOTES 'DINO head')."""
    head = _head()
    w = head.last_layer.weight
    assert not w.is_leaf and type(w.grad_fn).__name__ == "WeightNormInterfaceBackward0"
    first = _accumulate_grad_nodes(w.grad_fn)
    assert len(first) == 2
    assert {id(n.variable) for n in first} == {id(head.last_layer.weight_g), id(head.last_layer.weight_v)}
    del w
    x = torch.randn(3, 128)
    y = head(x)
    y.sum().backward()
    del y
    second = _accumulate_grad_nodes(head.last_layer.weight.grad_fn)
    y = head(x)
    third = _accumulate_grad_nodes(head.last_layer.weight.grad_fn)
    by_var = lambda nodes: {id(n.variable): n for n in nodes}
    a, b, c = by_var(first), by_var(second), by_var(third)
    assert set(a) == set(b) == set(c)
    for k in a:
        assert a[k] is b[k] and b[k] is c[k]


# ------------------------------------------------------------------------------------------------ C ABI without a device
def test_l2norm_ok_is_the_range():
    L = _lib.lib()
    for rows, D, want in [(1, 8, 1), (7, 264, 1), (65, 4096, 1), (1 << 20, 256, 1), (0, 256, 0), (1, 0, 0), (1, 4, 0),
                          (1, 260, 0), (1, 4104, 0), (1 << 31, 8, 0), (-1, 8, 0)]:
        assert L.octic_l2norm_ok(rows, D) == want, (rows, D)


def test_argument_validation_without_gpu():
    """Rejected arguments return negative codes before any launch (fake, aligned addresses: nothing is dereferenced)."""
    L = _lib.lib()
    p = lambda a: ctypes.c_void_p(a)
    A, B, C, D_ = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    ESHAPE, EALIGN, ENULL = -1, -2, -4
    fwd, bwd = L.octic_l2norm_rows_fwd, L.octic_l2norm_rows_bwd
    assert fwd(None, _lib.F32, 64, 4, 64, 1e-12, p(B), _lib.F32, 64, p(C), None) == ENULL
    assert fwd(p(A), _lib.F32, 64, 4, 64, 1e-12, p(B), _lib.F32, 64, None, None) == ENULL
    assert fwd(p(A), _lib.F32, 60, 4, 60, 1e-12, p(B), _lib.F32, 60, p(C), None) == ESHAPE          # D % 8
    assert fwd(p(A), _lib.F32, 4104, 4, 4104, 1e-12, p(B), _lib.F32, 4104, p(C), None) == ESHAPE    # D > 4096
    assert fwd(p(A), _lib.F32, 64, 0, 64, 1e-12, p(B), _lib.F32, 64, p(C), None) == ESHAPE          # no rows
    assert fwd(p(A), _lib.F32, 56, 4, 64, 1e-12, p(B), _lib.F32, 64, p(C), None) == ESHAPE          # ldx < D
    assert fwd(p(A), 7, 64, 4, 64, 1e-12, p(B), _lib.F32, 64, p(C), None) < 0                       # dtype
    assert fwd(p(A + 4), _lib.F32, 64, 4, 64, 1e-12, p(B), _lib.F32, 64, p(C), None) == EALIGN
    assert fwd(p(A), _lib.BF16, 68, 4, 64, 1e-12, p(B), _lib.BF16, 64, p(C), None) == EALIGN        # 136-byte rows
    assert bwd(p(A), _lib.F32, 64, None, _lib.F32, 64, p(C), 4, 64, 1e-12, p(D_), 64, None) == ENULL
    assert bwd(p(A), _lib.F32, 64, p(B), _lib.F32, 64, p(C), 4, 12, 1e-12, p(D_), 64, None) == ESHAPE
    assert bwd(p(A), _lib.F32, 64, p(B), _lib.F32, 64, p(C), 4, 64, 1e-12, p(D_), 32, None) == ESHAPE   # lddx < D
    assert bwd(p(A), _lib.F32, 64, p(B), _lib.F32, 64, p(C), 4, 64, 1e-12, p(D_ + 8), 64, None) == EALIGN
    prep, wbwd = L.octic_weight_norm_prep, L.octic_weight_norm_bwd
    assert prep(None, p(B), 8, 64, p(C), None, p(D_), None) == ENULL
    assert prep(p(A), p(B), 8, 64, p(C), None, None, None) == ENULL
    assert prep(p(A), p(B), 8, 60, p(C), None, p(D_), None) == ESHAPE                               # K % 8
    assert prep(p(A), p(B), 8, 4096, p(C), None, p(D_), None) == ESHAPE                             # K > 2048
    assert prep(p(A), p(B), 0, 64, p(C), None, p(D_), None) == ESHAPE
    assert prep(p(A), p(B), 12, 64, p(C), p(C + (1 << 16)), p(D_), None) == ESHAPE                  # W^T needs N % 8 == 0
    assert prep(p(A), p(B), 8, 64, p(C + 2), None, p(D_), None) == EALIGN
    assert wbwd(p(A), p(B), p(C), p(D_), 8, 64, None, p(D_ + 4096), None) == ENULL
    assert wbwd(p(A), p(B), p(C), p(D_), 8, 60, p(D_ + 4096), p(D_ + 8192), None) == ESHAPE
    assert wbwd(p(A + 4), p(B), p(C), p(D_), 8, 64, p(D_ + 4096), p(D_ + 8192), None) == EALIGN


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    from octic_vits_amd import ops
    x = torch.zeros(4, 64)
    for call in (lambda: ops.l2norm_rows(x), lambda: ops.l2norm_rows_bwd(x, x, torch.zeros(4)),
                 lambda: ops.weight_norm_prep(x, torch.ones(4, 1)),
                 lambda: ops.weight_norm_bwd(x, x, torch.ones(4, 1), torch.ones(4))):
        with pytest.raises(RuntimeError, match="GPU only"):
            call()
    assert ops.weight_norm_ok(65536, 256) and ops.weight_norm_ok(8, 64)
    assert not ops.weight_norm_ok(12, 64) and not ops.weight_norm_ok(8, 4096) and not ops.weight_norm_ok(8, 60)
    assert ops.l2norm_ok(40, 256) and not ops.l2norm_ok(40, 4100)


# ------------------------------------------------------------------------------------------------------------- routing
def test_dino_head_ok_refuses_what_the_engine_path_does_not_cover():
    """No GPU here: everything is a refusal - CPU tensors, float32 without autocast, BatchNorm, tracing, shapes outside
    dense_gemm_ok.  The device-independent half of the predicate (structure, shapes) is asked directly."""
    from octic_vits_amd import functional as OF, ops
    head = _head()
    x = torch.randn(4, 128)
    assert not OF.dino_head_ok(head, x)                                            # CPU tensor
    with torch.autocast("cpu", dtype=torch.bfloat16):
        assert not OF.dino_head_ok(head, x)                                        # ... under CPU autocast too
    assert not OF.dino_head_ok(head, x.to("meta"))                                 # not a CUDA tensor, no autocast
    # structure: BatchNorm in the MLP is not Linear (GELU Linear)*
    assert OF._dino_head_linears(_head(use_bn=True)) is None
    assert [m.in_features for m in OF._dino_head_linears(head)] == [128, 128, 128]
    assert len(OF._dino_head_linears(_head(nlayers=1))) == 1 and len(OF._dino_head_linears(_head(nlayers=2))) == 2
    # shapes: the bottleneck is the K of the prototype GEMM and must be >= 128 in steps of 64; prototypes % 64
    assert ops.dense_gemm_ok(40, 320, 128) and ops.dense_gemm_ok(40, 128, 320)
    assert not ops.dense_gemm_ok(40, 264, 64) and not ops.dense_gemm_ok(40, 264, 128) and not ops.dense_gemm_ok(40, 64, 128)
    # the recipe's widths, both directions, at the row counts of a 32-image step
    for rows in (40, 320 + 128, 64 + 128):
        for N, K in ((2048, 1280), (2048, 2048), (256, 2048), (65536, 256)):
            assert ops.dense_gemm_ok(rows, N, K) and ops.dense_gemm_ok(rows, K, N), (rows, N, K)
    # tracing: the predicate answers False while torch.compile traces (the stock composition is what gets compiled)
    seen = []

    def probe(t):
        seen.append(OF.dino_head_ok(head, t))
        return t + 1

    torch.compile(probe, backend="eager")(x)
    assert seen and not any(seen)


def test_switch_and_state_dict_keys():
    from octic_vits_amd import ssl as S
    assert isinstance(S.DINO_HEAD_HIP, bool)
    assert sorted(_head().state_dict()) == ["last_layer.weight_g", "last_layer.weight_v", "mlp.0.bias", "mlp.0.weight",
                                            "mlp.2.bias", "mlp.2.weight", "mlp.4.bias", "mlp.4.weight"]
    assert sorted(_head(nlayers=1).state_dict()) == ["last_layer.weight_g", "last_layer.weight_v", "mlp.bias", "mlp.weight"]
    # the stock composition is untouched on the CPU: same numbers as the plain restatement
    head = _head()
    x = torch.randn(5, 128)
    want = F.linear(F.normalize(head.mlp(x), dim=-1, p=2, eps=1e-12),
                    torch._weight_norm(head.last_layer.weight_v, head.last_layer.weight_g, 0))
    assert torch.equal(head(x), want)


# ------------------------------------------------------------------------------------------- the formulas, in float64
def l2norm_formulas(x, g, eps):
    """include/octic_hip.h: y, inv and dx of octic_l2norm_rows_fwd / _bwd."""
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    d = torch.where(n < eps, torch.full_like(n, eps), n)
    inv = 1.0 / d
    y = x / d
    yh = x * inv
    dx = torch.where(n < eps, g * inv, inv * (g - yh * (yh * g).sum(-1, keepdim=True)))
    return y, inv, dx


def weight_norm_formulas(v, g, dw):
    """include/octic_hip.h: W, norms of octic_weight_norm_prep and (dv, dg) of octic_weight_norm_bwd."""
    norms = v.pow(2).sum(1, keepdim=True).sqrt()
    r = 1.0 / norms
    w = g * v * r
    s = (dw * v).sum(1, keepdim=True)
    return w, norms, g * (r * dw - r ** 3 * s * v), s * r


def test_l2norm_formulas_are_autograd_of_normalize_in_float64():
    gen = torch.Generator().manual_seed(5)
    eps = 1e-12
    x = torch.randn(9, 64, dtype=torch.float64, generator=gen)
    x[2] = 0.0                                        # an exactly zero row
    x[5] = 1e-15 * torch.randn(64, dtype=torch.float64, generator=gen)     # a row below eps
    x[7] *= 1e-9                                      # small, but above eps
    g = torch.randn(9, 64, dtype=torch.float64, generator=gen)
    leaf = x.clone().requires_grad_(True)
    want = F.normalize(leaf, dim=-1, p=2, eps=eps)
    want.backward(g)
    y, inv, dx = l2norm_formulas(x, g, eps)
    assert float(x[5].norm()) < eps < float(x[7].norm())
    torch.testing.assert_close(y, want.detach(), rtol=1e-14, atol=0)
    torch.testing.assert_close(dx, leaf.grad, rtol=1e-12, atol=1e-12 * float(leaf.grad[[0, 1, 3, 4, 6, 8]].abs().max()))
    assert torch.equal(dx[2], g[2] * (1.0 / eps)) and torch.equal(y[2], torch.zeros(64, dtype=torch.float64))
    torch.testing.assert_close(dx[2], leaf.grad[2], rtol=1e-14, atol=0)               # the zero row: g / eps, nothing else
    torch.testing.assert_close(dx[5], leaf.grad[5], rtol=1e-14, atol=0)               # g / eps: no projection below eps
    assert float(inv[2]) == 1.0 / eps


def test_weight_norm_formulas_are_autograd_of_weight_norm_in_float64():
    gen = torch.Generator().manual_seed(6)
    v = torch.randn(24, 64, dtype=torch.float64, generator=gen)
    g = 0.5 + torch.rand(24, 1, dtype=torch.float64, generator=gen)
    dw = torch.randn(24, 64, dtype=torch.float64, generator=gen)
    lv, lg = v.clone().requires_grad_(True), g.clone().requires_grad_(True)
    want = torch._weight_norm(lv, lg, 0)
    want.backward(dw)
    w, norms, dv, dg = weight_norm_formulas(v, g, dw)
    torch.testing.assert_close(w, want.detach(), rtol=1e-14, atol=0)
    torch.testing.assert_close(norms[:, 0], v.norm(dim=1), rtol=1e-15, atol=0)
    torch.testing.assert_close(dv, lv.grad, rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(dg, lg.grad, rtol=1e-12, atol=1e-14)
