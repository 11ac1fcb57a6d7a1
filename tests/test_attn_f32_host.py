"""Host-side gates of the float32 attention (csrc/attn_f32.hip): the two C entry points exist and reject bad arguments
before any launch, the ABI version is unchanged, and the shape predicates keep the bf16 ones bf16-only.  No GPU needed."""
import os
import re

import torch

from octic_vits_amd import _lib, ops

A = 4096                       # a dummy 16-byte aligned address: rejected calls never dereference it


def _fwd(q=A, k=A, v=A, o=A, lse=A, B=2, H=3, T=17, hd=64, s=None, so=None, scale=0.125):
    s = s or (H * T * hd, T * hd, hd)
    so = so or s
    return _lib.lib().octic_attn_fwd_f32(q, k, v, o, lse, B, H, T, hd, *s, *so, scale, None)


def _bwd(ptrs=None, B=2, H=3, T=17, hd=64, s=None, so=None, sg=None, phase=3, scale=0.125):
    ptrs = ptrs or [A] * 10
    s = s or (H * T * hd, T * hd, hd)
    return _lib.lib().octic_attn_bwd_f32(*ptrs, B, H, T, hd, *s, *(so or s), *(sg or s), scale, phase, None)


def test_library_exports_the_f32_entry_points_and_keeps_the_abi_version():
    L = _lib.lib()
    assert hasattr(L, "octic_attn_fwd_f32") and hasattr(L, "octic_attn_bwd_f32")
    assert {"octic_attn_fwd_f32", "octic_attn_bwd_f32"} <= set(_lib.header_symbols())
    assert {"octic_attn_fwd_f32", "octic_attn_bwd_f32"} <= set(_lib._PROTOS)
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20


def test_fwd_rejects_bad_arguments_before_any_launch():
    assert _fwd(q=None) == -4 and _fwd(k=None) == -4 and _fwd(v=None) == -4 and _fwd(o=None) == -4
    for kw in (dict(T=0), dict(T=16385), dict(hd=72), dict(hd=144), dict(hd=0), dict(B=0), dict(H=0), dict(B=-1)):
        assert _fwd(**kw) == -1, kw
    assert _fwd(q=A + 4) == -2 and _fwd(o=A + 8) == -2
    assert _fwd(s=(3 * 17 * 64, 17 * 64, 66)) == -2               # a row stride of 66 floats breaks 16-byte rows
    assert _fwd(so=(3 * 17 * 64 + 2, 17 * 64, 64)) == -2


def test_bwd_rejects_bad_arguments_before_any_launch():
    for i in range(10):
        p = [A] * 10
        p[i] = None
        assert _bwd(ptrs=p) == -4, i
    for kw in (dict(T=0), dict(T=16385), dict(hd=72), dict(hd=144), dict(B=0), dict(H=0), dict(phase=0), dict(phase=4)):
        assert _bwd(**kw) == -1, kw
    for i in (0, 1, 2, 3, 4, 7, 8, 9):                            # q k v o dout dq dk dv (lse / delta are f32 scalars)
        p = [A] * 10
        p[i] = A + 4
        assert _bwd(ptrs=p) == -2, i
    assert _bwd(sg=(3 * 17 * 64, 17 * 64, 65)) == -2


def test_scale_must_be_positive_and_finite():
    for scale in (0.0, -0.125, float("inf"), float("nan")):
        assert _fwd(scale=scale) == -1, scale
        assert _bwd(scale=scale) == -1, scale


def test_f32_predicate_truth_table():
    f32 = torch.float32
    for T, hd in ((257, 80), (1370, 80), (1, 16), (16384, 128)):
        assert ops.attn_f32_supported(T, hd, f32), (T, hd)
        assert not ops.attn_f32_supported(T, hd, torch.bfloat16)
        assert not ops.attn_f32_supported(T, hd, torch.float16)
    assert not ops.attn_f32_supported(257, 72, f32)
    assert not ops.attn_f32_supported(257, 144, f32)
    assert not ops.attn_f32_supported(0, 64, f32)
    assert not ops.attn_f32_supported(16385, 64, f32)


def test_bf16_predicates_still_refuse_float32():
    assert not ops.attn_supported(577, 64, torch.float32)
    assert not ops.attn_packed_ok(1025, 160, 16, torch.float32)


def test_tile_constants_are_the_kernel_s_own():
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "attn_f32.hip")).read()
    waves = int(re.search(r"constexpr int kF32Waves = (\d+);", src).group(1))
    assert re.search(r"constexpr int kF32Rows = kF32Waves \* 32;", src)
    assert ops.ATTN_F32_ROWS == waves * 32
    assert ops.ATTN_F32_BLK == int(re.search(r"constexpr int kF32Blk = (\d+);", src).group(1))
