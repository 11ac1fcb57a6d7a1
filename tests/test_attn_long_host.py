"""Host-side gates of the long-sequence attention (csrc/attn_stream.hip): which shapes the HIP attention takes, how its
launches are named, and the routing knob that sends every T to the streaming kernels.  No GPU needed."""
import pytest
import torch

from octic_vits_amd import _lib, ops


def test_long_sequences_are_supported_in_bf16():
    assert ops.attn_supported(577, 64, torch.bfloat16)          # hybrid_deit_large_patch16 at 384^2
    assert ops.attn_supported(1025, 80, torch.bfloat16)         # hybrid_deit_huge_patch14 at 448^2
    assert ops.attn_supported(2049, 80, torch.bfloat16)
    assert ops.attn_supported(16384, 128, torch.bfloat16)
    assert ops.attn_packed_ok(1025, 160, 16, torch.bfloat16)    # head_dim 80 on packed rows
    assert ops.attn_packed_ok(577, 128, 16, torch.bfloat16)     # head_dim 64 on packed rows


def test_shapes_outside_the_kernels_stay_unsupported():
    assert not ops.attn_supported(577, 64, torch.float32)
    assert not ops.attn_supported(577, 64, torch.float16)
    assert not ops.attn_supported(577, 72, torch.bfloat16)
    assert not ops.attn_supported(577, 144, torch.bfloat16)
    assert not ops.attn_supported(16385, 64, torch.bfloat16)
    assert not ops.attn_supported(0, 64, torch.bfloat16)
    assert not ops.attn_packed_ok(1025, 160, 16, torch.float32)
    assert not ops.attn_packed_ok(16385, 160, 16, torch.bfloat16)
    assert not ops.attn_packed_ok(1025, 96, 16, torch.bfloat16)  # head_dim 48 on packed rows: no piece schedule


def test_long_sequences_name_the_streaming_launches():
    assert ops.attn_streams(321, 80) and ops.attn_streams(1025, 64)
    assert not ops.attn_streams(257, 80) and not ops.attn_streams(197, 64)
    assert ops._attn_fwd_name(1025, 80) == "attn_fwd_stream_kernel"
    assert ops._attn_fwd_name(257, 80) == "attn_fwd_kernel"
    phases = ops._attn_bwd_phases(1025, 80)
    assert [p[0] for p in phases] == [1, 2]
    assert [p[1] for p in phases] == ["attn_bwd_dq_stream_kernel", "attn_bwd_dkv_stream_kernel"]
    assert sum(p[3] for p in phases) == 14.0                      # 14 T^2 hd FLOP: dq (3 products) + dk, dv (4)
    assert ops._attn_bwd_phases(257, 80)[0][0] == 3               # T <= 320 keeps its routing


def test_stream_knob_round_trips():
    assert _lib.ROUTE_ATTN_STREAM == 11
    old = _lib.route_override(_lib.ROUTE_ATTN_STREAM, 1)
    try:
        assert old == 0
        assert ops.attn_streams(257, 80) and ops.attn_streams(197, 64)
        assert ops._attn_fwd_name(257, 80) == "attn_fwd_stream_kernel"
        assert ops._attn_bwd_phases(257, 80)[0][1] == "attn_bwd_dq_stream_kernel"
        assert _lib.route_override(_lib.ROUTE_ATTN_STREAM, 0) == 1
        assert not ops.attn_streams(257, 80)
    finally:
        _lib.route_override(_lib.ROUTE_ATTN_STREAM, 0)
    with pytest.raises(ValueError):                               # OCTIC_ROUTE_COUNT = 12
        _lib.route_override(12, 0)
