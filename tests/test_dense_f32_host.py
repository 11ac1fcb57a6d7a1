"""CPU-only checks of the float32 dense GEMM family (csrc/dense_f32.hip): the symbols, the accept-and-plan query, the error codes
the launchers return before any launch, and the seams of functional.py that choose between the kernels and the stock path."""
import ctypes
import os

import pytest
import torch

from octic_vits_amd import _lib, functional as OF, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["octic_dense_f32_nt", "octic_dense_f32_nn", "octic_dense_f32_tn", "octic_dense_gelu_bwd_f32",
       "octic_dense_f32_workspace_bytes", "octic_dense_f32_plan"]
NT, NN, TN = _lib.DENSE_F32_NT, _lib.DENSE_F32_NN, _lib.DENSE_F32_TN


def test_symbols_are_declared_exported_documented_and_the_abi_is_still_20():
    L = _lib.lib()
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    declared = _lib.header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in NEW:
        assert s in declared and s in _lib._PROTOS and hasattr(L, s) and s in text, s
    assert "dense_f32.hip" in __import__("octic_vits_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.mark.parametrize("op", [NT, NN, TN])
def test_plan_refuses_exactly_the_stated_shapes(op):
    ok = ops.dense_f32_plan
    assert ok(op, 5, 8, 12) is not None and ok(op, 1, 4, 4) is not None
    for M, N, K in ((5, 6, 8), (5, 8, 6), (5, 10, 12), (0, 8, 8), (-1, 8, 8), (5, 0, 8), (5, 8, 0)):
        assert ok(op, M, N, K) is None, (M, N, K)                      # N or K no multiple of 4, empty problems
    assert ok(op, 5, 8, 12, 12) is not None and ok(op, 5, 8, 12, 16) is not None
    assert ok(op, 5, 8, 12, 8) is None and ok(op, 5, 12, 8, 8) is None  # a stride below the longest operand row
    # 32-bit element offsets: (largest of M, N, K) * (largest stride) < 2^31
    assert ok(op, 2 ** 19 - 1, 4096, 4096) is not None                 # 2^31 - 4096
    assert ok(op, 2 ** 19, 4096, 4096) is None
    assert ok(op, 2 ** 19, 2048, 2048) is not None and ok(op, 2 ** 19, 2048, 2048, 4096) is None
    assert ok(op, 4, 2 ** 16, 2 ** 15) is None and ok(op, 2 ** 31, 4, 4) is None
    assert ops.dense_f32_plan(3, 5, 8, 12) is None and ops.dense_f32_plan(-1, 5, 8, 12) is None
    assert _lib.lib().octic_dense_f32_workspace_bytes(op, 5, 6, 8) == -1


def test_plan_accepts_the_vit_shapes_and_reports_the_launch():
    for D in (192, 384, 768, 1024, 1280, 1536):
        for width in (3 * D, 4 * D, 4096, 8192):
            for M in (1, 257, 64 * 257):
                for N, K in ((width, D), (D, width), (D, D)):
                    assert ops.dense_f32_ok(M, N, K), (M, N, K)
                    for op in (NT, NN, TN):
                        tr, tc, slabs, wgs = ops.dense_f32_plan(op, M, N, K)
                        rows, cols = (N, K) if op == TN else (M, N if op == NT else K)
                        assert tr > 0 and tc > 0 and slabs >= 1 and wgs == -(-rows // tr) * -(-cols // tc) * slabs
                        assert slabs == 1 or op == TN


def test_tn_slab_count_depends_on_the_shape_only_and_sizes_the_workspace():
    L = _lib.lib()
    seen = set()
    for M, N, K in ((514, 16, 16), (511, 16, 16), (64 * 257, 1280, 1280), (64 * 257, 3840, 1280), (64 * 257, 1280, 5120), (257, 1280, 1280)):
        a = ops.dense_f32_plan(TN, M, N, K)
        for ld in (0, max(N, K), max(N, K) + 8, 4 * max(N, K)):         # the stride does not enter
            assert ops.dense_f32_plan(TN, M, N, K, ld) == a
        _lib._PLANS.clear()                                            # ... nor does the call history
        assert ops.dense_f32_plan(TN, M, N, K) == a
        slabs = a[2]
        seen.add(slabs)
        need = L.octic_dense_f32_workspace_bytes(TN, M, N, K)
        assert need >= (slabs * (N * K + N) * 4 if slabs > 1 else 0) and need % 256 == 0 and need > 0
        assert slabs <= max(1, M // 256)                               # slabs of at least 256 rows
    assert 1 in seen and len(seen) > 2
    assert L.octic_dense_f32_workspace_bytes(NT, 514, 16, 16) == L.octic_dense_f32_workspace_bytes(NN, 514, 16, 16) == 256


def test_launchers_return_the_error_codes_before_any_launch():
    """No GPU here: a call that got as far as a launch would not return one of these codes."""
    L = _lib.lib()
    P, Q = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)      # aligned / misaligned non-null addresses, never read
    Z = ctypes.c_void_p(0)
    M, N, K = 5, 8, 12
    # NT (A, W, bias, M, N, K, lda, ldw, C, ldc, gelu, H, ldh, stream)
    nt = lambda A=P, W=P, b=Z, m=M, n=N, k=K, lda=K, ldw=K, C=P, ldc=N, gelu=0, H=Z, ldh=0: L.octic_dense_f32_nt(
        A, W, b, m, n, k, lda, ldw, C, ldc, gelu, H, ldh, None)
    assert nt(A=Z) == nt(W=Z) == nt(C=Z) == nt(gelu=1, H=Z, ldh=N) == -4
    assert nt(n=6) == nt(k=10) == nt(m=0) == nt(lda=K - 4) == nt(ldw=K - 4) == nt(ldc=N - 4) == nt(gelu=1, H=P, ldh=N - 4) == -1
    assert nt(A=Q) == nt(W=Q) == nt(C=Q) == nt(b=Q) == nt(gelu=1, H=Q, ldh=N) == nt(lda=K + 2) == nt(ldc=N + 1) == -2
    # NN (G, W, M, N, K, ldg, ldw, DX, ldx, stream)
    nn = lambda G=P, W=P, m=M, n=N, k=K, ldg=N, ldw=K, DX=P, ldx=K: L.octic_dense_f32_nn(G, W, m, n, k, ldg, ldw, DX, ldx, None)
    assert nn(G=Z) == nn(W=Z) == nn(DX=Z) == -4
    assert nn(n=6) == nn(k=10) == nn(m=0) == nn(ldg=N - 4) == nn(ldw=K - 4) == nn(ldx=K - 4) == -1
    assert nn(G=Q) == nn(W=Q) == nn(DX=Q) == nn(ldg=N + 2) == -2
    # TN (G, X, M, N, K, ldg, ldx, DW, ldw, db, workspace, workspace_bytes, stream)
    tn = lambda G=P, X=P, m=M, n=N, k=K, ldg=N, ldx=K, DW=P, ldw=K, db=Z, ws=P, nb=1 << 20: L.octic_dense_f32_tn(
        G, X, m, n, k, ldg, ldx, DW, ldw, db, ws, nb, None)
    assert tn(G=Z) == tn(X=Z) == tn(DW=Z) == -4
    assert tn(n=6) == tn(k=10) == tn(m=0) == tn(ldg=N - 4) == tn(ldx=K - 4) == tn(ldw=K - 4) == -1
    assert tn(G=Q) == tn(X=Q) == tn(DW=Q) == tn(ws=Q) == tn(ldx=K + 2) == -2
    assert ops.dense_f32_plan(TN, 514, 16, 16)[2] > 1
    assert tn(m=514, n=16, k=16, ldg=16, ldx=16, ldw=16, ws=Z) == -4      # several slabs need the workspace ...
    assert tn(m=514, n=16, k=16, ldg=16, ldx=16, ldw=16, nb=256) == -5    # ... all of it
    # GELU backward (h, g, dh, partials, db, rows, d, stream)
    gb = lambda h=P, g=P, dh=P, part=Z, db=Z, rows=M, d=N: L.octic_dense_gelu_bwd_f32(h, g, dh, part, db, rows, d, None)
    assert gb(h=Z) == gb(g=Z) == gb(dh=Z) == gb(db=P, part=Z) == -4
    assert gb(d=6) == gb(d=0) == gb(rows=-1) == -1
    assert gb(h=Q) == gb(g=Q) == gb(dh=Q) == gb(part=Q, db=P) == -2
    assert gb(rows=0) == 0


def test_functional_seams_pick_the_stock_path_off_the_gpu_in_bf16_and_with_the_switch_off(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a float32 kernel was chosen")
    for name in ("dense_f32_nt", "dense_f32_nn", "dense_f32_tn", "dense_gelu_bwd_f32"):
        monkeypatch.setattr(ops, name, boom)
    g = torch.Generator().manual_seed(0)
    x, w, b, gy = (torch.randn(s, generator=g) for s in ((6, 12), (8, 12), (8,), (6, 8)))
    assert OF.DENSE_F32_HIP is True
    for dt in (torch.float32, torch.bfloat16):                          # CPU tensors, either dtype
        xx, ww, bb, gg = x.to(dt), w.to(dt), b.to(dt), gy.to(dt)
        assert not OF.dense_f32_hip_ok(6, 8, 12, xx, ww)
        assert torch.equal(OF._linear_lib(xx, ww, bb), torch.nn.functional.linear(xx, ww, bb))
        assert torch.equal(OF._mm_lib(gg, ww), gg @ ww)
        # (the stock weight gradient sums row slabs: the same product in another order)
        torch.testing.assert_close(OF._wgrad_lib(gg, xx), (gg.t() @ xx).float(), rtol=2e-2, atol=2e-2)

    class FakeCuda(torch.Tensor):                                       # a tensor that says it lives on the GPU
        is_cuda = True
    fx, fw = x.as_subclass(FakeCuda), w.as_subclass(FakeCuda)
    assert OF.dense_f32_hip_ok(6, 8, 12, fx, fw)                        # float32 on the GPU: the kernels ...
    assert not OF.dense_f32_hip_ok(6, 8, 12, fx.bfloat16().as_subclass(FakeCuda), fw)      # ... not for bf16 ...
    assert not OF.dense_f32_hip_ok(6, 8, 12, fx, fw.t().contiguous().as_subclass(FakeCuda).t())   # ... nor a column-strided operand ...
    assert not OF.dense_f32_hip_ok(6, 8, 10, fx[:, :10], fw[:, :10])    # ... nor for a shape the plan refuses ...
    monkeypatch.setattr(OF, "DENSE_F32_HIP", False)
    assert not OF.dense_f32_hip_ok(6, 8, 12, fx, fw)                    # ... nor with the switch off
