"""CPU-only side of the weight-gradient entry points that skip dropped samples (octic_dense_wgrad_tn_skip / _tn_pair_skip): the
prototypes, the OCTIC_WGRAD_SKIP switch, which per-sample factors travel to the kernel, and rejections that come back before any
launch."""
import ctypes

import pytest
import torch

from octic_vits_amd import _lib

SKIP = ["octic_dense_wgrad_tn_skip", "octic_dense_wgrad_tn_pair_skip"]


def test_skip_entry_points_are_declared_prototyped_and_exported():
    L = _lib.lib()
    assert set(SKIP) <= set(_lib.header_symbols()) and set(SKIP) <= set(_lib._PROTOS)
    for name in SKIP:
        plain = name[:-len("_skip")]
        assert hasattr(L, name) and hasattr(L, plain)
        args, base = _lib._PROTOS[name][1], _lib._PROTOS[plain][1]
        # the plain argument list with sample_scale, rows_per_sample in front of workspace, stream
        assert list(args) == list(base[:-2]) + [ctypes.c_void_p, ctypes.c_int] + list(base[-2:]), name
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20          # additions only


def test_switch_is_read_from_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_WGRAD_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_WGRAD_SKIP") is True    # on by default
    monkeypatch.setenv("OCTIC_WGRAD_SKIP", "0")
    assert OF._skip_from_env("OCTIC_WGRAD_SKIP") is False
    monkeypatch.setenv("OCTIC_WGRAD_SKIP", "1")
    assert OF._skip_from_env("OCTIC_WGRAD_SKIP") is True
    assert isinstance(OF.WGRAD_SKIP_DROPPED, bool)


def test_only_per_sample_gpu_factors_reach_the_kernel(monkeypatch):
    import octic_vits_amd.functional as OF
    from octic_vits_amd import ops
    rs = torch.tensor([2.0, 0.0, 2.0])
    monkeypatch.setattr(OF, "WGRAD_SKIP_DROPPED", True)
    assert OF.wgrad_skip_scale(None, 17, 51) is None                 # eval, drop_path 0
    assert OF.wgrad_skip_scale(rs, 17, 51) is None                   # a CPU tensor: no kernel reads it
    meta = torch.empty(3, device="meta")                             # passes for a GPU tensor as far as the shape rules go
    monkeypatch.setattr(type(meta), "is_cuda", property(lambda self: True), raising=False)
    assert OF.wgrad_skip_scale(meta, 17, 51) is not None
    assert OF.wgrad_skip_scale(meta, 17, 52) is None                 # rps * B != M
    assert OF.wgrad_skip_scale(meta, 1, 3) is None                   # one factor per ROW: a ragged row tensor
    assert OF.wgrad_skip_scale(meta, 17, 51, rows_to=object()) is None
    assert OF.wgrad_skip_scale(meta.double(), 17, 51) is None
    monkeypatch.setattr(OF, "WGRAD_SKIP_DROPPED", False)
    assert OF.wgrad_skip_scale(meta, 17, 51) is None
    assert ops._sample_scale(None, 17, 51, rs, "dense_wgrad_tn") == (None, 0)
    assert ops._sample_scale(rs, 17, 51, rs, "dense_wgrad_tn") == (rs, 17)
    for bad in (rs.double(), rs[:2], torch.zeros(6)[::2]):
        with pytest.raises(ValueError, match="sample_scale"):
            ops._sample_scale(bad, 17, 51, rs, "dense_wgrad_tn")


def test_rejections_come_back_before_any_launch():
    L = _lib.lib()
    p, ss, odd = 4096, 8192, 8194
    one = lambda M, s, rps: L.octic_dense_wgrad_tn_skip(p, p, M, 256, 256, 256, 256, p, s, rps, p, None)
    two = lambda M, s, rps: L.octic_dense_wgrad_tn_pair_skip(p, p, 768, 768, 256, p, p, p, 256, 256, 256, p, M, 256, s, rps, p, None)
    for f in (one, two):
        assert f(2056, ss, 0) == -1 and f(2056, ss, -3) == -1        # a mask needs rows_per_sample > 0
        assert f(2056, ss, 256) == -1                                # ... that divides M
        assert f(2056, odd, 257) == -2                               # sample_scale must be 4-byte aligned
        assert f(0, ss, 257) == -1                                   # the plain calls' refusals come first
    # without a mask rows_per_sample is not looked at; the plain entry points are the _skip ones with NULL
    assert L.octic_dense_wgrad_tn_skip(p + 2, p, 2056, 256, 256, 256, 256, p, None, 0, p, None) == -2
    assert L.octic_dense_wgrad_tn(p + 2, p, 2056, 256, 256, 256, 256, p, p, None) == -2
    assert L.octic_dense_wgrad_tn_skip(None, p, 2056, 256, 256, 256, 256, p, ss, 257, p, None) == -4
