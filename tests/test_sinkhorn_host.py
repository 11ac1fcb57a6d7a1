"""CPU-only: the Sinkhorn-Knopp passes of csrc/ssl_loss.hip are declared, exported and bound, refuse bad arguments before any
launch, and ssl._sinkhorn routes to them only where they apply.  No compute call is made (there is no GPU here)."""
import os

import pytest
import torch

from octic_vits_amd import _lib

SYMBOLS = ["octic_sinkhorn_slabs", "octic_sinkhorn_protos", "octic_sinkhorn_rows", "octic_sinkhorn_final"]
ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4
P = 4096                                   # a 16-byte aligned, never dereferenced address


def test_symbols_are_declared_exported_bound_and_documented():
    declared = _lib.header_symbols()
    L = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    for s in SYMBOLS:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert L.octic_abi_version() == 20


def test_slab_plan_edges():
    """32 rows a slab until 256 slabs, then the slabs grow: the edges tests/test_sinkhorn_gpu.py runs rows around."""
    L = _lib.lib()
    assert [L.octic_sinkhorn_slabs(r) for r in (1, 32, 33, 64, 65, 8192, 8193, 8224, 1 << 20)] == [1, 1, 2, 2, 3, 256, 249, 250, 256]
    assert L.octic_sinkhorn_slabs(0) == ESHAPE and L.octic_sinkhorn_slabs(-3) == ESHAPE and L.octic_sinkhorn_slabs(1 << 31) == ESHAPE


def _calls(L, x=P, dtype=_lib.BF16, ld=64, rows=4, K=64, vec=P, small=P):
    """Every pass with the same logits arguments; vec stands for the f32 [K] / [rows, K] operands, small for the f32 [rows] ones."""
    return [L.octic_sinkhorn_protos(x, dtype, ld, 1.0, small, small, vec, vec, rows, K, None),
            L.octic_sinkhorn_rows(x, dtype, ld, 1.0, vec, small, small, rows, K, None),
            L.octic_sinkhorn_final(x, dtype, ld, 1.0, vec, vec, rows, K, None)]


def test_argument_validation_returns_negative_codes_without_a_launch():
    L = _lib.lib()
    assert _calls(L, K=12, ld=16) == [ESHAPE] * 3                      # K % 8
    assert _calls(L, K=0) == [ESHAPE] * 3
    assert _calls(L, rows=0) == [ESHAPE] * 3                           # no round to run
    assert _calls(L, rows=-1) == [ESHAPE] * 3
    assert _calls(L, ld=56) == [ESHAPE] * 3                            # row stride below K
    assert _calls(L, x=P + 4) == [EALIGN] * 3                          # misaligned logits
    assert _calls(L, ld=68) == [EALIGN] * 3                            # bf16 rows off the 16-byte grid
    assert _calls(L, ld=66, dtype=_lib.F32) == [EALIGN] * 3           # f32 rows off the 16-byte grid
    assert _calls(L, vec=P + 8) == [EALIGN] * 3                        # misaligned u / r / out
    assert _calls(L, x=0) == [ENULL] * 3
    assert _calls(L, dtype=_lib.U8) == [EDTYPE] * 3
    # required outputs; u is nullable in the row passes, the slab workspace where there is one slab
    assert L.octic_sinkhorn_protos(P, _lib.BF16, 64, 1.0, 0, P, P, P, 4, 64, None) == ENULL
    assert L.octic_sinkhorn_protos(P, _lib.BF16, 64, 1.0, P, 0, P, P, 4, 64, None) == ENULL
    assert L.octic_sinkhorn_protos(P, _lib.BF16, 64, 1.0, P, P, P, 0, 4, 64, None) == ENULL
    assert L.octic_sinkhorn_protos(P, _lib.BF16, 64, 1.0, P, P, 0, P, 33, 64, None) == ENULL      # two slabs need partials
    assert L.octic_sinkhorn_rows(P, _lib.BF16, 64, 1.0, P, 0, P, 4, 64, None) == ENULL
    assert L.octic_sinkhorn_rows(P, _lib.BF16, 64, 1.0, P, P, 0, 4, 64, None) == ENULL
    assert L.octic_sinkhorn_final(P, _lib.BF16, 64, 1.0, P, 0, 4, 64, None) == ENULL


def test_ops_refuse_cpu_tensors():
    from octic_vits_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sinkhorn_rows(torch.zeros(2, 8), 1.0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sinkhorn_final(torch.zeros(2, 8), 1.0, torch.ones(8))


def _meta(*shape, dtype=torch.bfloat16):
    """A tensor that says it is on the GPU without one: the predicate reads only device, dtype and shape."""
    return torch.empty(*shape, dtype=dtype, device="meta")


def test_routing_predicate(monkeypatch):
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ssl as S
    # stand-in for `is_cuda` where there is no device: everything else of loss_rows_ok is the real rule
    monkeypatch.setattr(OF, "loss_rows_ok", lambda t: t.device.type in ("cuda", "meta") and t.dtype in (torch.float32, torch.bfloat16)
                        and t.shape[-1] % 8 == 0)
    assert S.FUSED_LOSS_ROWS is True
    assert S.sinkhorn_fused_ok(_meta(5, 64), 3) and S.sinkhorn_fused_ok(_meta(1, 8, dtype=torch.float32), 1)
    assert not S.sinkhorn_fused_ok(_meta(5, 64), 0)                    # no iteration: exp / total only
    assert not S.sinkhorn_fused_ok(_meta(2, 5, 64), 3)                 # 3-D
    assert not S.sinkhorn_fused_ok(_meta(0, 64), 3)                    # no rows (and no process group)
    assert not S.sinkhorn_fused_ok(_meta(5, 60), 3)                    # K % 8
    assert not S.sinkhorn_fused_ok(_meta(5, 64, dtype=torch.float16), 3)
    assert not S.sinkhorn_fused_ok(torch.zeros(5, 64), 3)              # CPU
    monkeypatch.setattr(S, "FUSED_LOSS_ROWS", False)
    assert not S.sinkhorn_fused_ok(_meta(5, 64), 3)


def test_a_rank_without_rows_launches_nothing_and_returns_no_rows():
    """In a process group a rank whose batch has no rows takes the fused path for its collectives only: no kernel (this runs
    without a GPU), an empty f32 result."""
    from octic_vits_amd import ssl as S
    out = S._sinkhorn_fused(torch.empty(0, 64, dtype=torch.bfloat16), 0.05, 3)
    assert out.shape == (0, 64) and out.dtype == torch.float32


def test_cpu_and_unfused_calls_run_the_composition(monkeypatch):
    """On inputs the predicate refuses, _sinkhorn is the stock composition bit for bit and never reaches the ops."""
    from octic_vits_amd import ops
    from octic_vits_amd import ssl as S

    def boom(*a, **k):
        raise AssertionError("a Sinkhorn kernel wrapper was called")
    for name in ("sinkhorn_rows", "sinkhorn_protos", "sinkhorn_final"):
        monkeypatch.setattr(ops, name, boom)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(6, 64, generator=g) * 0.5

    def stock(x, temp, B, n):
        Q = torch.exp(x.float() / temp).t()
        K = Q.shape[0]
        Q = Q / torch.sum(Q)
        for _ in range(n):
            Q = Q / torch.sum(Q, dim=1, keepdim=True) / K
            Q = Q / torch.sum(Q, dim=0, keepdim=True) / B
        return (Q * B).t()
    for n in (0, 3):
        assert torch.equal(S.DINOLoss(64).sinkhorn_knopp_teacher(x, 0.05, n_iterations=n), stock(x, 0.05, 6, n))
    cnt = torch.tensor([6])
    got = S.iBOTPatchLoss(64).sinkhorn_knopp_teacher(x, 0.05, cnt)
    assert torch.equal(got, stock(x, 0.05, torch.tensor([6]), 3)) and cnt.item() == 6
    x3 = x.view(2, 3, 64)
    with pytest.raises(RuntimeError):
        S.DINOLoss(64).sinkhorn_knopp_teacher(x3, 0.05)                # the composition's own refusal of 3-D (.t()), unchanged
