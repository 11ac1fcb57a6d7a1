"""Host side of the octic MLP's sample masks (no GPU): the OCTIC_LINEAR_SKIP switch, which per-sample factors travel to the
kernels, the new prototypes, and that the header and the library still name the same symbols."""
import os
import re
import subprocess

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("octic_linear_d8_fwd_skip", "octic_gelu_d8_fwd_skip", "octic_gelu_d8_bwd_skip", "octic_attn_skip_plan")


def test_switch_reads_the_environment(monkeypatch):
    import octic_vits_amd.functional as OF
    monkeypatch.delenv("OCTIC_LINEAR_SKIP", raising=False)
    assert OF._skip_from_env("OCTIC_LINEAR_SKIP") is True    # on by default
    monkeypatch.setenv("OCTIC_LINEAR_SKIP", "0")
    assert OF._skip_from_env("OCTIC_LINEAR_SKIP") is False
    monkeypatch.setenv("OCTIC_LINEAR_SKIP", "1")
    assert OF._skip_from_env("OCTIC_LINEAR_SKIP") is True
    assert isinstance(OF.LINEAR_SKIP_DROPPED, bool)


class _Factors:
    """What linear_skip_scale reads of a per-sample factor tensor, without a GPU."""

    def __init__(self, n, cuda=True, dtype=torch.float32, dim=1, contiguous=True):
        self.is_cuda, self.dtype, self._n, self._dim, self._contiguous = cuda, dtype, n, dim, contiguous

    def dim(self):
        return self._dim

    def numel(self):
        return self._n

    def is_contiguous(self):
        return self._contiguous

    def detach(self):
        return self


def test_which_factors_travel(monkeypatch):
    """The conditions of wgrad_skip_scale."""
    import octic_vits_amd.functional as OF
    monkeypatch.setattr(OF, "LINEAR_SKIP_DROPPED", True)
    good = _Factors(3)
    assert OF.linear_skip_scale(None, 17, 51) is None                # eval, drop_path 0
    assert OF.linear_skip_scale(torch.tensor([2.0, 0.0, 2.0]), 17, 51) is None    # a CPU tensor: no kernel reads it
    assert OF.linear_skip_scale(good, 17, 51) is good
    assert OF.linear_skip_scale(good, 17, 52) is None                # rps * B != M
    assert OF.linear_skip_scale(good, 1, 3) is None                  # one factor per ROW: a ragged row tensor
    assert OF.linear_skip_scale(good, 17, 51, rows_to=object()) is None   # compact rows
    assert OF.linear_skip_scale(_Factors(3, dtype=torch.float64), 17, 51) is None
    assert OF.linear_skip_scale(_Factors(3, dim=2), 17, 51) is None
    assert OF.linear_skip_scale(_Factors(3, contiguous=False), 17, 51) is None
    monkeypatch.setattr(OF, "LINEAR_SKIP_DROPPED", False)
    assert OF.linear_skip_scale(good, 17, 51) is None


# Kernels that skip a sample whose factor is 0 (DESIGN.md 'Routing rules'): a80::fwd_os_kernel - the one-shot head_dim-80 forward
# at NINE 32-token tiles, launches of up to 512 samples; every single-pass backward of csrc/attn80_bwd.hip; the resident dq + dkv
# pair of csrc/attention.hip.  Not: fwd_oss_kernel, the online forward, attention.hip's forwards, the streaming and f32 kernels.
def _expected_skip(B, T, hd):
    from octic_vits_amd import _lib
    fwd, _, bwd, _ = _lib.attn_plan(T, hd)
    fwd_skips = fwd == _lib.ATTN_FWD_A80_ONESHOT and (T + 31) // 32 == 9 and B <= 512
    return fwd_skips and bwd in (_lib.ATTN_BWD_SINGLE, _lib.ATTN_BWD_PAIR)


def test_predicate_follows_the_attention_plan():
    """ops.attn_skips_dropped for every T in 1 .. 320 at head_dim 64 and 80, by default and under each OCTIC_ROUTE_ATTN_*
    override: true exactly where both planned kernels are in the list above."""
    from octic_vits_amd import _lib, ops
    knobs = [(None, 0), (_lib.ROUTE_ATTN_LEGACY, 1), (_lib.ROUTE_ATTN_ONLINE, 1), (_lib.ROUTE_ATTN_BWD_PAIR, 1),
             (_lib.ROUTE_ATTN_STREAM, 1)]
    true_at = {}
    for knob, value in knobs:
        if knob is not None:
            _lib.route_override(knob, value)
        try:
            for hd in (64, 80):
                for T in range(1, 321):
                    got = ops.attn_skips_dropped(64, T, hd)
                    assert got == _expected_skip(64, T, hd), (knob, hd, T)
                    if got:
                        true_at.setdefault(knob, []).append((hd, T))
            assert ops.attn_skips_dropped(512, 257, 80) == _expected_skip(512, 257, 80)
            assert ops.attn_skips_dropped(513, 257, 80) is False       # past the forward's order table
        finally:
            if knob is not None:
                _lib.route_override(knob, 0)
    assert true_at[None] == [(80, 257), (80, 258)]                   # ViT-H/14 at 224 x 224 and its neighbour, nothing else
    assert true_at[_lib.ROUTE_ATTN_BWD_PAIR] == [(80, 257), (80, 258)]    # the resident pair skips too
    assert _lib.ROUTE_ATTN_LEGACY not in true_at and _lib.ROUTE_ATTN_ONLINE not in true_at and _lib.ROUTE_ATTN_STREAM not in true_at
    # the packed layout's strides (ViT-H: c = 160) and the unfused backward
    assert ops.attn_skips_dropped(64, 257, 80, ld=(3840, 1280, 3840)) is True
    before = ops.ATTN_BWD_FUSED
    ops.ATTN_BWD_FUSED = False
    try:
        assert ops.attn_skips_dropped(64, 257, 80) is True            # phases 1 and 2: the resident pair
    finally:
        ops.ATTN_BWD_FUSED = before
    assert ops.attn_skips_dropped(64, 257, 80, dtype=_lib.F32) is False


def test_the_mlp_hands_no_mask_without_its_fused_tail(monkeypatch):
    """MlpD8._sample_mask is None on the CPU, without a residual (nobody multiplies the branch by rs then), under the compacted
    batch and with the switch off - before any tensor is looked at."""
    import octic_vits_amd.d8_layers as L
    import octic_vits_amd.functional as OF
    mlp = L.MlpD8(64, 256)
    x = OF.Octic(torch.zeros(2, 5, 64), 8)
    rs = torch.tensor([2.0, 0.0])
    assert mlp._sample_mask(x, x.packed, rs) is None                 # CPU tensors
    assert mlp._sample_mask(x, None, rs) is None
    monkeypatch.setattr(L, "COMPACT_DROP_PATH", True)
    assert mlp._sample_mask(x, x.packed, rs) is None
    monkeypatch.setattr(L, "COMPACT_DROP_PATH", False)
    monkeypatch.setattr(OF, "LINEAR_SKIP_DROPPED", False)
    assert mlp._sample_mask(x, x.packed, rs) is None


def test_prototypes_and_abi():
    from octic_vits_amd import _lib
    header = open(os.path.join(ROOT, "include", "octic_hip.h")).read()
    assert f"#define OCTIC_ABI_VERSION {_lib.ABI_VERSION}" in header      # additions only: the number stays
    for name in NEW:
        assert name in _lib._PROTOS
        assert re.search(r"\bint " + name + r"\(", header), name
    # the skip calls take the plain call's arguments, then (sample_scale, rows_per_sample), then the stream
    for plain, skip in (("octic_linear_d8_fwd", NEW[0]), ("octic_gelu_d8_fwd", NEW[1]), ("octic_gelu_d8_bwd", NEW[2])):
        a, b = _lib._PROTOS[plain][1], _lib._PROTOS[skip][1]
        assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 2 and b[-1] == a[-1]


def test_library_exports_what_the_header_declares():
    so = os.path.join(ROOT, "octic_vits_amd", "liboctic_hip.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (octic_\w+)", out))
    for name in NEW:
        assert name in exported, name
