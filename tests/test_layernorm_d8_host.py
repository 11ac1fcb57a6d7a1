"""LayerNormD8 kernel matrix, host side: the float64 references of tests/golden/ln_d8_cases.py against the oracle, and the
case tables against the list of kernel instances csrc/layernorm.hip holds.  Runs anywhere."""
import numpy as np
import pytest
import torch

import ln_d8_cases as L
from oracle import octic_ref as R


def _rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("c", [8, 72, 160])
@pytest.mark.parametrize("affine", L.AFFINE)
@pytest.mark.parametrize("kind", ["normal", "const_row"])
def test_references_agree_with_the_oracle(c, affine, kind):
    """ln_ref / ln_bwd_ref (closed formulas) = LayerNormD8 in float64 + autograd, 1e-12 of each tensor's largest entry."""
    M = 9
    x, g, dres = L.make_x(M, c, kind).double(), L.make_g(M, c).double(), L.make_g(M, c, "res").double()
    alpha5, beta = L.make_affine(c)
    if affine == "none":
        alpha5 = None
    if affine != "alpha_beta":
        beta = None
    ln = R.LayerNormD8(8 * c, eps=L.EPS, elementwise_affine=alpha5 is not None, bias=beta is not None).double()
    if alpha5 is not None:
        with torch.no_grad():
            for n, a in zip(("A1", "A2", "B1", "B2", "E"), alpha5):
                getattr(ln.scaling, "alpha_" + n).copy_(a.double())
            if beta is not None:
                ln.scaling.beta.copy_(beta.double())
    xs = [t.clone().requires_grad_(True) for t in L.unpack5(x[None], c)]
    ys = ln(tuple(xs))
    torch.autograd.backward(ys, list(L.unpack5(g[None], c)))
    y, mean, rstd = L.ln_ref(x.numpy(), alpha5, beta)
    dx, dal, dbeta = L.ln_bwd_ref(g.numpy(), x.numpy(), alpha5, dres.numpy())
    assert _rel(y, L.pack5(ys).detach().numpy()) < 1e-12
    assert _rel(dx - dres.numpy(), L.pack5([t.grad for t in xs]).numpy()) < 1e-12
    # the statistics: segment means and 1 / std as the oracle's forward forms them
    seg = L.segments(c)
    want_mean = np.stack([x.numpy()[:, lo:hi].mean(1) for lo, hi, _, _ in seg], 1)
    assert np.abs(mean - want_mean).max() < 1e-12 * max(1.0, np.abs(want_mean).max())
    var = lambda t: t.var(dim=-1, unbiased=False)
    u = L.unpack5(x, c)
    S = var(u[0]) + var(u[1]) + var(u[2]) + var(u[3]) + var(u[4]).mean(-1) + L.EPS
    assert _rel(rstd, (1.0 / (R.SQRT2_OVER_4 * torch.sqrt(S))).numpy()) < 1e-12
    if alpha5 is not None:
        for n, d in zip(("A1", "A2", "B1", "B2", "E"), dal):
            assert _rel(d, getattr(ln.scaling, "alpha_" + n).grad.numpy()) < 1e-12, n
        if beta is not None:
            assert _rel(dbeta, ln.scaling.beta.grad.numpy()) < 1e-12
    else:
        # no parameters to differentiate: d alpha of a unit alpha is sum g * xhat, d beta is sum g
        xh = (L.pack5(ys).detach().numpy())
        assert _rel(np.concatenate(dal[:4]), (g.numpy() * xh).sum(0)[:4 * c]) < 1e-12
    assert _rel(dbeta, g.numpy()[:, :c].sum(0)) < 1e-12


def test_tables_reach_every_kernel_instance():
    got = L.reached()
    missing = {k: sorted(v - got.get(k, set())) for k, v in L.REQUIRED.items() if v - got.get(k, set())}
    assert not missing, f"kernel instances no case launches: {missing}"
    extra = {k: sorted(v - L.REQUIRED.get(k, set())) for k, v in got.items() if v - L.REQUIRED.get(k, set())}
    assert not extra, f"route() names instances the library does not have: {extra}"
    assert sum(len(v) for v in L.REQUIRED.values()) == 8 + 8 + 3 + 5 + 5 + 6 * 4


def test_route_rule():
    assert L.route(128, True, "bf16") == ("ln_bwd_g8_wide", 4)              # the ViT-L train step
    assert L.route(192, True, "bf16") == ("ln_bwd_g8_bf16_narrow", 6)
    assert L.route(192, True, "bf16", cast=True) == ("refused", 0)
    assert L.route(48, True, "bf16", cast=True) == ("refused", 0)
    assert L.route(32, False, "bf16", cast=True) == ("refused", 0)
    assert L.route(160, True, "bf16", cast=True, mask=True) == ("ln_bwd_g8_wide_mask", 5)
    assert L.route(160, False) == ("ln_fwd_tuple", 5) and L.route(32, False, "f32") == ("ln_bwd_tuple_f32", 2)
    assert L.route(72, True) == ("ln_fwd_pk", 4) and L.route(168, True, "f32") == ("ln_bwd_pk_f32", 8)
    assert L.route(264, True) == ("refused", 0) and L.route(12, True) == ("refused", 0)
    assert [L.pick_nv(c) for c in (8, 64, 72, 128, 136, 160, 168, 256, 264)] == [2, 2, 4, 4, 5, 5, 8, 8, 0]
    for c, nv, whole, lanes in ((72, 4, 2, 16), (168, 8, 5, 16)):
        # `whole` chunks of all 64 lanes, one more for `lanes` lanes only, and the other chunks of the instance beyond the row
        assert L.pick_nv(c) == nv and 2 * c == 64 * whole + lanes and whole + 1 < nv
    assert [L.bwd_blocks(M) for M in (1, 8, 9, 2048, 2049, 4100)] == [1, 1, 2, 256, 256, 256]
    for nblk in L.FINISH_NBLK:
        assert 1 <= nblk <= L.BWD_CAP
