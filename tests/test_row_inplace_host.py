"""CPU-only: who may be written into (functional.OwnedStreamGrad), the switch, and the refusals of the in-place entry points that
happen before any launch."""
import ctypes

import pytest
import torch


@pytest.fixture
def OF():
    import octic_vits_amd.functional as OF
    before = (OF.ROW_INPLACE, OF.ROW_SKIP_DROPPED)
    OF.ROW_INPLACE = OF.ROW_SKIP_DROPPED = True
    OF.STREAM_GRADS.clear()
    yield OF
    OF.ROW_INPLACE, OF.ROW_SKIP_DROPPED = before
    OF.STREAM_GRADS.clear()


def test_the_switch_reads_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_ROW_INPLACE", raising=False)
    assert OF._skip_from_env("OCTIC_ROW_INPLACE") is True
    monkeypatch.setenv("OCTIC_ROW_INPLACE", "0")
    assert OF._skip_from_env("OCTIC_ROW_INPLACE") is False


def _chain(OF, log, offer=True, other=False):
    """Two nodes in a row: the upper one (runs second in the backward) asks for the cotangent the lower one returned."""

    class Lower(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2.0

        @staticmethod
        def backward(ctx, g):
            log["incoming_taken"] = OF.STREAM_GRADS.take(g)               # the caller's cotangent: never offered
            dx = g * 2.0                                                  # allocated here
            log["dx_ptr"] = dx.data_ptr()
            if offer:
                OF.STREAM_GRADS.offer(dx)
            return dx

    class Upper(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x + 1.0

        @staticmethod
        def backward(ctx, g):
            log["same_buffer"] = g.data_ptr() == log["dx_ptr"]
            log["taken"] = OF.STREAM_GRADS.take(g.clone() if other else g)
            log["taken_twice"] = OF.STREAM_GRADS.take(g)
            return g

    x = torch.randn(4, 8, requires_grad=True)
    return x, Lower.apply(Upper.apply(x))


def test_only_the_offered_buffer_of_the_running_pass_is_taken(OF):
    log = {}
    x, y = _chain(OF, log)
    g = torch.randn(4, 8)
    keep = g.clone()
    y.backward(g)
    assert log == {"incoming_taken": False, "dx_ptr": log["dx_ptr"], "same_buffer": True, "taken": True, "taken_twice": False}
    assert torch.equal(g, keep)
    assert OF.STREAM_GRADS.storage is None                                # nothing outlives the pass


def test_a_copy_is_not_the_buffer_and_an_unoffered_one_is_nobodys(OF):
    log = {}
    _, y = _chain(OF, log, other=True)
    y.backward(torch.randn(4, 8))
    assert log["taken"] is False and log["taken_twice"] is False          # (the entry is consumed by the failed take)
    log = {}
    _, y = _chain(OF, log, offer=False)
    y.backward(torch.randn(4, 8))
    assert log["same_buffer"] is True and log["taken"] is False


def test_an_entry_dies_with_its_pass_and_with_the_switches(OF):
    t = torch.randn(3, 4)
    OF.STREAM_GRADS.offer(t)                                              # outside a backward pass: not recorded
    assert OF.STREAM_GRADS.storage is None and OF.STREAM_GRADS.take(t) is False
    log = {}
    _, y = _chain(OF, log)
    y.backward(torch.randn(4, 8))
    assert OF.STREAM_GRADS.storage is None
    for name in ("ROW_INPLACE", "ROW_SKIP_DROPPED"):
        setattr(OF, name, False)
        log = {}
        _, y = _chain(OF, log)
        y.backward(torch.randn(4, 8))
        assert log["taken"] is False, name
        setattr(OF, name, True)


def test_in_place_entry_points_refuse_before_any_launch():
    """No mask: OCTIC_ENULL (-4); rows that are no whole samples: OCTIC_ESHAPE (-1); no factors in the forward: OCTIC_ENULL."""
    from octic_vits_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(4096)
    n = ctypes.c_void_p(0)
    tail = lambda ss, rows, rps: L.octic_dense_layernorm_bwd_tail_inplace(p, p, p, p, p, n, p, n, n, 1, p, n, rows, 256, ss, rps, n)
    assert tail(n, 12, 3) == -4
    assert tail(p, 12, 5) == -1 and tail(p, 12, 0) == -1
    assert L.octic_dense_resid_layernorm_fwd_skip(p, p, _lib.BF16, n, n, 3, p, p, _lib.BF16, n, n, p, 12, 256, 1e-6, n) == -4
    v = _lib.OcticView()
    for i in range(5):
        v.ptr[i] = 4096 + 4 * 32 * i if i < 4 else 4096 + 4 * 32 * 4
        v.ld[i] = 8 * 32
    cast = lambda ss, rps, c=32: L.octic_layernorm_d8_bwd_cast_inplace(ctypes.byref(v), ctypes.byref(v), p, None, ctypes.byref(v), p,
                                                                       12, c, n, 1, p, ss, rps, n)
    assert cast(n, 3) == -4
    assert cast(p, 5) == -1
    assert cast(p, 3, c=192) == -1                                        # beyond the wide kernel's chunk counts
