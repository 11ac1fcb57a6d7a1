"""Every ops launcher that takes a stochastic-depth mask (sample_scale / dropped) refuses a malformed one with a ValueError
before any launch, and without a mask it runs the same `_skip` entry point with a null pointer: its outputs are those of an
all-ones mask bit for bit.

Two samples of 37 rows everywhere (attention: two samples of 37 tokens).  The three malformed masks are chosen so that even a
launcher that forgot to look at them would read only memory the mask owns: float64 of the right count, float32 one entry too
long, a [::2] view of float32 twice the length.  Device and dtype on fake tensors: tests/test_wgrad_skip_host.py and
tests/test_attn_skip_host.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, RPS = 2, 37
M = B * RPS
C = 32                           # channels per irrep of the octic row kernels and GEMM input
H, HD = 2, 80                    # attention heads (packed: c = 10 H)
NAN = float("nan")


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _randn(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g, device=DEV).to(dtype)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _flat(out):
    """The tensors of a launcher's result, nested lists and Nones flattened away."""
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [t for o in out for t in _flat(o)]


# ---- one builder per launcher: operands made once -> run(mask) -> its outputs ----------------------------------------------
def _gelu(backward):
    from octic_vits_amd import ops
    g = _gen(1)
    x, dy = _randn(g, M, 8 * C, dtype=torch.bfloat16), _randn(g, M, 8 * C, dtype=torch.bfloat16)

    def run(ss):
        y = _nan(M, 8 * C)
        if backward:
            ops.gelu_bwd(ops.pview(dy, C), ops.pview(x, C), ops.pview(y, C), M, C, x.dtype, x, sample_scale=ss, rows_per_sample=RPS)
        else:
            ops.gelu_fwd(ops.pview(x, C), ops.pview(y, C), M, C, x.dtype, x, sample_scale=ss, rows_per_sample=RPS)
        return y
    return run


def _layernorm(cast):
    from octic_vits_amd import ops
    g = _gen(2)
    x = _randn(g, B, RPS, 8 * C) * 2 + 0.3
    alpha = [torch.rand(C if i < 4 else 2 * C, generator=g, device=DEV) + 0.5 for i in range(5)]
    _, stats = ops.layernorm_fwd(x, alpha, None, 1e-5, torch.bfloat16, C)
    gy, dres = _randn(g, B, RPS, 8 * C, dtype=torch.bfloat16), _randn(g, B, RPS, 8 * C)
    rs = torch.tensor([2.0, 0.0], device=DEV)

    def run(ss):
        if cast:
            return ops.layernorm_bwd_cast(gy, x, stats, alpha, dres, C, rs, RPS, sample_scale=ss, rows_per_sample=RPS)
        return ops.layernorm_bwd(gy, x, stats, alpha, dres, C, sample_scale=ss, rows_per_sample=RPS)
    return run


def _dense_tail():
    from octic_vits_amd import ops
    g, d = _gen(3), 256
    x = _randn(g, M, d) * 1.5 + 0.25
    w, gamma = _randn(g, d) * 0.5 + 1.0, _randn(g, d) * 0.1
    _, stats = ops.dense_layernorm_fwd(x, w, None, 1e-6, torch.bfloat16)
    gy, dres, yb = _randn(g, M, d, dtype=torch.bfloat16), _randn(g, M, d), _randn(g, M, d, dtype=torch.bfloat16)
    rs = torch.tensor([0.0, 2.0], device=DEV)
    return lambda ss: ops.dense_layernorm_bwd_tail(gy, x, w, stats, dres, yb, gamma, rs, RPS, sample_scale=ss, rows_per_sample=RPS)


def _colsum():
    from octic_vits_amd import ops
    gy = _randn(_gen(4), M, 256, dtype=torch.bfloat16)
    return lambda ss: ops.dense_colsum(gy, ss, RPS)


def _wgrad(pair):
    from octic_vits_amd import ops
    g, K = _gen(5), 256
    dy0, x0 = _randn(g, M, 768 if pair else 256, dtype=torch.bfloat16), _randn(g, M, K, dtype=torch.bfloat16)
    dy1, x1 = _randn(g, M, 256, dtype=torch.bfloat16), _randn(g, M, K, dtype=torch.bfloat16)
    if pair:
        return lambda ss: ops.dense_wgrad_tn_pair(dy0, x0, dy1, x1, sample_scale=ss, rows_per_sample=RPS)
    return lambda ss: ops.dense_wgrad_tn(dy0, x0, sample_scale=ss, rows_per_sample=RPS)


def _dense_gemm(mode):
    from octic_vits_amd import ops
    g, N, K = _gen(6), 256, 128
    a, b = _randn(g, M, K, dtype=torch.bfloat16), (_randn(g, N, K) * K ** -0.5).to(torch.bfloat16)
    bias, h = _randn(g, N), _randn(g, M, N, dtype=torch.bfloat16)
    if mode == 3:                # gelu'(h) * c and its column sums: the launch sizes them from the plan in force
        return lambda ss: ops.dense_gemm_nt(a, b, 3, h=h, want_colsum=True, tokens=RPS, sample_scale=ss, rows_per_sample=RPS)
    return lambda ss: ops.dense_gemm_nt(a, b, 0, bias=bias, tokens=RPS, sample_scale=ss, rows_per_sample=RPS)


def _linear(contract):
    from octic_vits_amd import ops
    g, cout = _gen(7), 64
    x = _randn(g, M, 8 * C, dtype=torch.bfloat16)
    w32 = [_randn(g, *s) * 0.1 for s in [(cout, C)] * 4 + [(2 * cout, 2 * C)]]
    wb, _ = ops.linear_prep(w32, None, C, cout, torch.bfloat16, want_wb=True)
    bias = _randn(g, cout) if contract == "sample_scale" else None       # a plain `dropped` launch takes no bias

    def run(ss):
        y = _nan(M, 8 * cout)
        ops.linear_fwd(ops.pview(x, C), wb, bias, ops.pview(y, cout), M, C, cout, torch.bfloat16, torch.bfloat16, x,
                       **{contract: ss, "skip_rps" if contract == "sample_scale" else "dropped_rps": RPS})
        return y
    return run


def _attn(packed, backward):
    from octic_vits_amd import ops
    g, scale = _gen(8), HD ** -0.5
    if packed:
        c = 10 * H
        qkv, do = _randn(g, B, RPS, 3 * 8 * c, dtype=torch.bfloat16) * 0.7, _randn(g, B, RPS, 8 * c, dtype=torch.bfloat16)
        o, lse = ops.attn_fwd_packed(qkv, H, c, scale)
        if backward:
            return lambda ss: ops.attn_bwd_packed(qkv, o, do, lse, H, c, scale, out=_nan(*qkv.shape), sample_scale=ss)
        return lambda ss: ops.attn_fwd_packed(qkv, H, c, scale, out=_nan(*o.shape), sample_scale=ss)
    qkv, do = _randn(g, B, RPS, 3, H, HD, dtype=torch.bfloat16), _randn(g, B, RPS, H, HD, dtype=torch.bfloat16).permute(0, 2, 1, 3)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    o, lse = ops.attn_fwd(q, k, v, scale, out=_nan(B, RPS, H, HD).permute(0, 2, 1, 3))

    def run(ss):
        if not backward:
            return ops.attn_fwd(q, k, v, scale, out=_nan(B, RPS, H, HD).permute(0, 2, 1, 3), sample_scale=ss)
        dqkv = _nan(*qkv.shape)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        ops.attn_bwd(q, k, v, o, do, lse, scale, dq, dk, dv, sample_scale=ss)
        return dqkv
    return run


LAUNCHERS = {
    "gelu_fwd": lambda: _gelu(False), "gelu_bwd": lambda: _gelu(True),
    "layernorm_bwd": lambda: _layernorm(False), "layernorm_bwd_cast": lambda: _layernorm(True),
    "dense_layernorm_bwd_tail": _dense_tail, "dense_colsum": _colsum,
    "dense_wgrad_tn": lambda: _wgrad(False), "dense_wgrad_tn_pair": lambda: _wgrad(True),
    "dense_gemm_nt": lambda: _dense_gemm(0), "dense_gemm_nt colsum": lambda: _dense_gemm(3),
    "linear_fwd sample_scale": lambda: _linear("sample_scale"), "linear_fwd dropped": lambda: _linear("dropped"),
    "attn_fwd": lambda: _attn(False, False), "attn_bwd": lambda: _attn(False, True),
    "attn_fwd_packed": lambda: _attn(True, False), "attn_bwd_packed": lambda: _attn(True, True),
}


@pytest.mark.parametrize("name", list(LAUNCHERS))
def test_a_malformed_mask_is_refused_and_no_mask_is_the_all_ones_mask(name):
    run = LAUNCHERS[name]()
    malformed = {"float64": torch.ones(B, dtype=torch.float64, device=DEV),
                 "one entry too long": torch.ones(B + 1, device=DEV),
                 "strided view": torch.ones(2 * B, device=DEV)[::2]}
    for what, bad in malformed.items():
        with pytest.raises(ValueError, match="sample_scale"):
            run(bad)                                                 # (let through, it would read B floats the mask owns)
    masked = _flat(run(torch.ones(B, device=DEV)))
    plain = _flat(run(None))
    torch.cuda.synchronize()
    assert masked and len(masked) == len(plain)
    for i, (a, b) in enumerate(zip(masked, plain)):
        assert bool(torch.isfinite(a.float()).all()), f"{name}: output {i} is not finite"
        assert torch.equal(a, b), f"{name}: output {i}, {int((a != b).sum())} elements differ between no mask and all ones"
