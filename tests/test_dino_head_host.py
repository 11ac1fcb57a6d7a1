"""Input rows of the DINO / iBOT heads (csrc/dino_head.hip) without a GPU: octic_head_rows' refusals before any launch (fake
pointers, as in test_abi_symbols.test_argument_validation_without_gpu), the routing predicate on CPU tensors, and
``ssl.DINOHead`` on CPU tensors - today's composition bitwise, the reference's numbers of tests/golden/ssl_pieces.npz, the
state-dict keys."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases
from octic_vits_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P = 1 << 20                      # a fake, 16-byte aligned device address: nothing is launched on a refused call
ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4


def _hr(seg=P, nseg=3, rows=10, D=64, dt=_lib.F32, out=P, ldo=64, scatter=0):
    return _lib.lib().octic_head_rows(seg, nseg, rows, D, dt, out, ldo, scatter, None)


def test_head_rows_refuses_before_any_launch():
    for scatter in (0, 1):
        for kw in (dict(nseg=0), dict(nseg=5), dict(rows=0), dict(D=0), dict(D=12, ldo=16), dict(ldo=56), dict(D=(1 << 20) + 8, ldo=1 << 21)):
            assert _hr(scatter=scatter, **kw) == ESHAPE, kw
        assert _hr(scatter=scatter, out=P + 8) == EALIGN
        assert _hr(scatter=scatter, ldo=66) == EALIGN
        assert _hr(scatter=scatter, dt=_lib.BF16, ldo=68) == EALIGN
        assert _hr(scatter=scatter, seg=None) == ENULL and _hr(scatter=scatter, out=None) == ENULL
        assert _hr(scatter=scatter, dt=_lib.U8) == EDTYPE


def _stock(head, x):
    """dinov2/layers/dino_head.py:36-41, op by op."""
    x = head.mlp(x)
    x = F.normalize(x, dim=-1, p=2, eps=1e-6 if x.dtype == torch.float16 else 1e-12)
    return head.last_layer(x)


def test_head_is_the_stock_composition_on_cpu_bitwise_and_matches_the_reference_numbers():
    from octic_vits_amd import ssl as S
    import ssl_case as C
    want = np.load(os.path.join(GOLD, "ssl_pieces.npz"))
    head = cases.fill_parameters(S.DINOHead(in_dim=C.D, out_dim=C.K, hidden_dim=40, bottleneck_dim=24, nlayers=3))
    assert list(head.state_dict()) == ["mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias", "mlp.4.weight", "mlp.4.bias",
                                       "last_layer.weight_g", "last_layer.weight_v"]
    hx = cases.randn("ssl.head.x", 7, C.D).requires_grad_(True)
    assert S.HEAD_HIP is True
    hy = head(hx)
    (hy * cases.randn("ssl.head.cot", 7, C.K)).sum().backward()
    got = {n: p.grad.clone() for n, p in head.named_parameters()}
    gx = hx.grad.clone()
    assert np.allclose(hy.detach().numpy(), want["head.y"], rtol=1e-5, atol=1e-6)
    assert np.allclose(gx.numpy(), want["head.gx"], rtol=1e-4, atol=1e-6)
    for n, g in got.items():
        assert np.allclose(g.numpy(), want["head.gpar." + n], rtol=1e-4, atol=1e-6), n
    for p in head.parameters():
        p.grad = None
    hx2 = hx.detach().clone().requires_grad_(True)
    hy2 = _stock(head, hx2)
    (hy2 * cases.randn("ssl.head.cot", 7, C.K)).sum().backward()
    assert torch.equal(hy, hy2) and torch.equal(gx, hx2.grad)
    for n, p in head.named_parameters():
        assert torch.equal(got[n], p.grad), n


@pytest.mark.parametrize("kw", [dict(nlayers=1), dict(nlayers=2), dict(use_bn=True), dict(mlp_bias=False)])
def test_every_head_variant_keeps_its_keys_and_the_stock_arm_on_cpu(kw):
    from octic_vits_amd import ssl as S
    torch.manual_seed(0)
    head = S.DINOHead(in_dim=128, out_dim=192, hidden_dim=128, bottleneck_dim=128, **kw)
    lin = [k for k in head.state_dict() if k.startswith("mlp")]
    assert [k for k in head.state_dict() if k.startswith("last_layer")] == ["last_layer.weight_g", "last_layer.weight_v"]
    assert ("mlp.weight" in lin) == (kw.get("nlayers") == 1)
    x = torch.randn(5, 128)
    assert torch.equal(head(x), _stock(head, x))


def test_cpu_sources_keep_the_stock_assembly():
    """The routing predicate refuses CPU tensors, and SSLMetaArch._head_rows then answers None: the caller runs new_zeros +
    index_select + copy_ + cat as before."""
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ssl as S
    cls, patches, idx = torch.randn(4, 64), torch.randn(4, 9, 64), torch.arange(5)
    specs = ((None, 0), (idx, 4))
    assert not OF.head_rows_ok(12, specs, (cls, patches))
    assert S.SSLMetaArch._head_rows(12, (cls, None, 0), (patches, idx, 4)) is None
