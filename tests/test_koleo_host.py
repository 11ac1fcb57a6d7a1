"""KoLeo kernels (csrc/koleo.hip) without a GPU: the routing query at the edges of its range, the entry points' refusals before
any launch (fake pointers, as in test_abi_symbols.test_argument_validation_without_gpu), and the torch arm of
``ssl.KoLeoLoss`` on CPU tensors - the reference's numbers of tests/golden/ssl_pieces.npz and ``forward_groups`` against the
per-chunk losses."""
import os

import numpy as np
import pytest
import torch

import cases
from octic_vits_amd import _lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_MAX = 256
P = 1 << 20                      # a fake, 16-byte aligned device address: nothing is launched on a refused call


@pytest.mark.parametrize("groups,n,D,want", [
    (1, 1, 64, 0), (1, 2, 64, 1), (1, N_MAX, 64, 1), (1, N_MAX + 1, 64, 0),
    (2, 16, 0, 0), (2, 16, 8, 1), (2, 16, 12, 0), (2, 16, 4096, 1), (2, 16, 4104, 0),
    (0, 16, 64, 0), (-1, 16, 64, 0), (3, 64, 1280, 1),
    ((1 << 31) // 16 - 1, 16, 64, 1), ((1 << 31) // 16, 16, 64, 0),       # groups * n < 2^31
])
def test_koleo_ok_at_the_edges_of_the_range(groups, n, D, want):
    assert _lib.lib().octic_koleo_ok(groups, n, D) == want


def _fwd(x=P, dt=_lib.F32, ldx=64, groups=2, n=4, D=64, term=P, nn=P, inv=P, dist=P):
    return _lib.lib().octic_koleo_fwd(x, dt, ldx, groups, n, D, 1e-8, term, nn, inv, dist, None)


def _bwd(x=P, dt=_lib.F32, ldx=64, groups=2, n=4, D=64, gterm=P, nn=P, inv=P, dist=P, dx=P, lddx=64):
    return _lib.lib().octic_koleo_bwd(x, dt, ldx, groups, n, D, 1e-8, gterm, nn, inv, dist, dx, lddx, None)


def test_forward_refuses_before_any_launch():
    for kw in (dict(n=1), dict(n=N_MAX + 1), dict(D=12, ldx=16), dict(D=0), dict(D=4104, ldx=4104), dict(groups=0),
               dict(ldx=56)):
        assert _fwd(**kw) == -1, kw
    assert _fwd(x=P + 4) == -2
    assert _fwd(dt=_lib.F32, ldx=66) == -2                  # 264-byte rows
    assert _fwd(dt=_lib.BF16, ldx=68) == -2                 # 136-byte rows
    for name in ("x", "term", "nn", "inv", "dist"):
        assert _fwd(**{name: None}) == -4, name
    assert _fwd(dt=_lib.U8) == -3


def test_backward_refuses_before_any_launch():
    for kw in (dict(n=1), dict(n=N_MAX + 1), dict(D=12, ldx=16, lddx=16), dict(groups=0), dict(ldx=56), dict(lddx=56)):
        assert _bwd(**kw) == -1, kw
    assert _bwd(x=P + 8) == -2
    assert _bwd(dx=P + 8) == -2
    assert _bwd(ldx=66) == -2
    assert _bwd(lddx=66) == -2
    assert _bwd(dt=_lib.BF16, lddx=68) == -2
    for name in ("x", "gterm", "nn", "inv", "dist", "dx"):
        assert _bwd(**{name: None}) == -4, name


def test_cpu_tensors_keep_the_torch_arm_and_the_reference_numbers():
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ssl as S
    want = np.load(os.path.join(GOLD, "ssl_pieces.npz"))
    D = want["koleo.gx"].shape[1]
    x = cases.randn("ssl.koleo.x", 10, D).requires_grad_(True)
    assert not OF.koleo_rows_ok(x, 1)
    loss = S.KoLeoLoss()(x)
    loss.backward()
    assert np.allclose(loss.detach().numpy().reshape(1), want["koleo.loss"], rtol=1e-5, atol=1e-5)
    scale = max(1.0, float(np.abs(want["koleo.gx"]).max()))
    assert np.allclose(x.grad.numpy(), want["koleo.gx"], rtol=1e-5, atol=1e-5 * scale)


def test_forward_groups_on_cpu_is_the_chunk_losses_bitwise():
    from octic_vits_amd import ssl as S
    kl = S.KoLeoLoss()
    x = cases.randn("koleo.host.groups", 12, 32)
    a = x.clone().requires_grad_(True)
    got = kl.forward_groups(a, 2)
    assert got.shape == (2,)
    sum(got.unbind(0)).backward()
    b = x.clone().requires_grad_(True)
    want = [kl(p) for p in b.chunk(2)]
    sum(want).backward()
    assert torch.equal(got.detach(), torch.stack(want).detach())
    assert torch.equal(a.grad, b.grad)
    three = kl.forward_groups(x, 3)
    assert torch.equal(three, torch.stack([kl(p) for p in x.chunk(3)]))
