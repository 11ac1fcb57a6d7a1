"""CPU-only side of the attention entry points that skip dropped samples (octic_attn_*_skip): the prototypes, the
OCTIC_ATTN_SKIP switch, which per-sample factors travel to the kernels, and rejections that come back before any launch."""
import ctypes

import pytest
import torch

from octic_vits_amd import _lib

SKIP = ["octic_attn_fwd_skip", "octic_attn_bwd_skip", "octic_attn_fwd_packed_skip", "octic_attn_bwd_packed_skip"]


def test_skip_entry_points_are_declared_prototyped_and_exported():
    L = _lib.lib()
    assert set(SKIP) <= set(_lib.header_symbols()) and set(SKIP) <= set(_lib._PROTOS)
    for name in SKIP:
        plain = name[:-len("_skip")]
        assert hasattr(L, name) and hasattr(L, plain)
        args, base = _lib._PROTOS[name][1], _lib._PROTOS[plain][1]
        # the plain argument list with the sample_scale pointer in front of the stream
        assert list(args) == list(base[:-1]) + [ctypes.c_void_p, base[-1]], name
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20          # additions only


def test_switch_is_read_from_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_ATTN_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_ATTN_SKIP") is True    # on by default
    monkeypatch.setenv("OCTIC_ATTN_SKIP", "0")
    assert OF._skip_from_env("OCTIC_ATTN_SKIP") is False
    monkeypatch.setenv("OCTIC_ATTN_SKIP", "1")
    assert OF._skip_from_env("OCTIC_ATTN_SKIP") is True
    assert isinstance(OF.ATTN_SKIP_DROPPED, bool)


def test_only_per_sample_gpu_factors_reach_the_kernels(monkeypatch):
    import octic_vits_amd.functional as OF
    rs = torch.tensor([2.0, 0.0, 2.0])
    monkeypatch.setattr(OF, "ATTN_SKIP_DROPPED", True)
    assert OF.skip_scale(None, 3) is None
    assert OF.skip_scale(rs, 3) is None                              # a CPU tensor: no kernel reads it
    monkeypatch.setattr(OF, "ATTN_SKIP_DROPPED", False)
    assert OF.skip_scale(rs, 3) is None
    from octic_vits_amd import ops
    assert ops._sample_scale(None, 1, 3, rs, "attn_fwd") == (None, 0)
    assert ops._sample_scale(rs, 1, 3, rs, "attn_fwd")[0] is rs
    for bad in (rs.double(), rs[:2], torch.zeros(6)[::2]):
        with pytest.raises(ValueError, match="sample_scale"):
            ops._sample_scale(bad, 1, 3, rs, "attn_fwd")


def test_rejections_come_back_before_any_launch():
    L = _lib.lib()
    p, ss, odd = 4096, 8192, 8194
    st = (2 * 257 * 480, 80, 480)
    fwd = lambda q, T, hd, s: L.octic_attn_fwd_skip(q, p, p, p, p, 2, 2, T, hd, *st, *st, 0.1, s, None)
    assert fwd(None, 257, 80, ss) == -4
    assert fwd(p, 257, 72, ss) == -1
    assert fwd(p, 0, 80, ss) == -1
    assert fwd(p, 257, 80, odd) == -2                                # sample_scale must be 4-byte aligned
    bwd = lambda T, phase, s: L.octic_attn_bwd_skip(*([p] * 10), 2, 2, T, 80, *st, *st, *st, 0.1, phase, s, None)
    assert bwd(257, 0, ss) == -1 and bwd(257, 3, odd) == -2
    fp = lambda c, s: L.octic_attn_fwd_packed_skip(p, p, p, 2, 2, 257, c, 480, 160, 0.1, s, None)
    assert fp(18, ss) == -1 and fp(20, odd) == -2
    bp = lambda c, ld_g, s: L.octic_attn_bwd_packed_skip(*([p] * 6), 2, 2, 257, c, 480, 160, ld_g, 0.1, 3, s, None)
    assert bp(18, 480, ss) == -1 and bp(20, 472, ss) == -2 and bp(20, 480, odd) == -2
