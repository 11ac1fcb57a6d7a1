"""octic_dense_gemm_nt_tokens_adaptive on the GPU (csrc/dense_gemm.hip dense_nt_adaptive_kernel): a masked one-round launch of
the 320-wide tile that chooses its tile width on the device.  Either width gives every output element the same MFMA sequence
over K, so everything here is torch.equal / bit patterns on random bf16 operands with a bias, against the UNMASKED launch of the
same call (the 320-wide tile): every row of every kept sample equal, class-token rows included; the patch rows of dropped
samples +0; everything finite.  No tolerance anywhere.

Per-image panels and the 320-wide plan are forced for the small batches (the launch model takes neither that small) and every
case asserts through octic_dense_gemm_plan_adaptive / octic_dense_gemm_order_adaptive that the adaptive kernel takes the launch
and which width it runs, so no case passes on the other path."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOK = 257

MASKS = {
    1: [[1], [0]],
    3: [[1, 0, 1]],
    5: [[0, 1, 0, 0, 1]],
    17: [[1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]],
}


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


@contextlib.contextmanager
def routed(tile=0, image=0):
    L = lib()
    try:
        L.route_override(L.ROUTE_DENSE_TILE, tile)
        L.route_override(L.ROUTE_DENSE_IMAGE, image)
        yield
    finally:
        L.route_override(L.ROUTE_DENSE_TILE, 0)
        L.route_override(L.ROUTE_DENSE_IMAGE, 0)


@pytest.fixture
def narrow_switch():
    import octic_vits_amd.functional as OF
    before = OF.DENSE_NARROW_DROPPED
    OF.DENSE_NARROW_DROPPED = True
    yield OF
    OF.DENSE_NARROW_DROPPED = before


_OPERANDS = {}


def operands(M, N, K):
    """Random bf16 operands and an f32 bias of one shape, shared by the cases of that shape and never modified; with them the
    unmasked launch's output per routing (computed once)."""
    key = (M, N, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 4:
            _OPERANDS.clear()
        g = torch.Generator(device=DEV).manual_seed(104729 * M + 17 * N + K)
        a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        b = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=DEV)
        _OPERANDS[key] = (a, b, bias, {})
    return _OPERANDS[key]


def scale_of(keep):
    return torch.tensor([2.0 if k else 0.0 for k in keep], dtype=torch.float32, device=DEV)


def chosen_width(B, N, K, keep):
    sc = np.ascontiguousarray([2.0 if k else 0.0 for k in keep], dtype=np.float32)
    width = ctypes.c_int(0)
    g = lib().lib().octic_dense_gemm_order_adaptive(B * TOK, N, K, 0, TOK, sc.ctypes.data, TOK, 1 << 16, None, None, None,
                                                    ctypes.addressof(width))
    assert g > 0, "the adaptive kernel does not take this launch"
    return width.value


def is_plus_zero(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


def dead_panel_rows(M, image, keep):
    """Rows of the row panels all of whose samples are dropped, by the panel geometry (per-image: the 256 patch rows of image
    tm; classic: rows 256 tm .. 256 tm + 255)."""
    rows = torch.zeros(M, dtype=torch.bool, device=DEV)
    for tm in range(M // TOK if image else -(-M // 256)):
        m0 = tm * TOK + 1 if image else tm * 256
        m1 = min(m0 + 256, M)
        if not any(keep[b] for b in range(m0 // TOK, (m1 - 1) // TOK + 1)):
            rows[m0:m1] = True
    return rows


def check_case(B, N, K, keep, force, tile=5, image=1):
    """One masked launch through the adaptive entry point against the unmasked launch of the same routing; returns the width the
    adaptive kernel ran, or None where it does not take the launch (K = 192: no per-image panels, the class-token kernel needs
    K % 128 == 0 - the call is then octic_dense_gemm_nt_tokens_skip on classic panels and must hold the same contract)."""
    o, L = ops(), lib()
    M = B * TOK
    a, b, bias, wants = operands(M, N, K)
    with routed(tile=tile + force, image=image):
        eligible, grid = o.dense_plan_adaptive(M, N, K, 0, TOK, TOK)[:2]
        assert eligible == (K % 128 == 0)
        per_image = o.dense_plan(M, N, K, 0, TOK)[2]
        assert o.dense_plan(M, N, K, 0, TOK)[0] == 320 and per_image == eligible
        if eligible:
            assert grid == 5 * B
        width = chosen_width(B, N, K, keep) if eligible else None
        if (tile, image) not in wants:
            wants[(tile, image)] = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK)
        want = wants[(tile, image)]
        got = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=scale_of(keep), rows_per_sample=TOK)
    rowkeep = torch.tensor(keep, dtype=torch.bool, device=DEV).repeat_interleave(TOK)
    assert torch.equal(got[rowkeep], want[rowkeep]), "rows of kept samples differ from the unmasked launch"
    if per_image:
        cls = torch.zeros(M, dtype=torch.bool, device=DEV)
        cls[::TOK] = True
        assert torch.equal(got[cls], want[cls]), "class-token rows differ"
    dead = dead_panel_rows(M, per_image, keep)
    assert bool(dead.any()) == (not all(keep)) or not per_image
    if bool(dead.any()):
        assert is_plus_zero(got[dead]), "rows of dropped samples' panels are not +0"
    assert bool(torch.isfinite(got.float()).all())
    if force and eligible:
        assert width == (320 if force == L.DENSE_ADAPT_WIDE else 256)
    return width


@pytest.mark.parametrize("force", ("rule", "wide", "narrow"))
@pytest.mark.parametrize("K", (128, 192, 256))
@pytest.mark.parametrize("B", (1, 3, 5, 17))
def test_small_batches_equal_the_unmasked_launch(B, K, force, narrow_switch):
    """K = 128 / 256 (two / four K-tiles: the guarded and the steady K loop) run the adaptive kernel; K = 192 forwards."""
    L = lib()
    f = {"rule": 0, "wide": L.DENSE_ADAPT_WIDE, "narrow": L.DENSE_ADAPT_NARROW}[force]
    for keep in MASKS[B]:
        width = check_case(B, 1280, K, keep, f)
        if force == "rule" and K != 192:
            assert width == 256                                            # 5 B <= 256: always narrow at these sizes


BOUNDARY = {"51-kept": [1] * 51 + [0] * 13, "52-kept": [1] * 52 + [0] * 12, "all-kept": [1] * 64, "all-dropped": [0] * 64}


@pytest.mark.parametrize("force", ("rule", "wide", "narrow"))
@pytest.mark.parametrize("name", list(BOUNDARY))
def test_decision_boundary_at_64_panels(name, force, narrow_switch):
    """B 64, N 1280, K 128 - the plan the model chooses by itself (nothing forced but the adaptive choice): narrow while at most
    51 panels are live (5 x 51 = 255 tiles on 256 CUs), wide from 52; all dropped is narrow, all kept wide.  The kept samples
    are spread over the batch so that both bitmap bytes and every group of 8 panels hold dead and live panels."""
    L = lib()
    f = {"rule": 0, "wide": L.DENSE_ADAPT_WIDE, "narrow": L.DENSE_ADAPT_NARROW}[force]
    keep = BOUNDARY[name]
    keep = [keep[(b * 37) % 64] for b in range(64)]                        # a fixed permutation (37 is coprime to 64)
    assert sum(keep) == sum(BOUNDARY[name])
    width = check_case(64, 1280, 128, keep, f, tile=0, image=0)
    if force == "rule":
        assert width == {"51-kept": 256, "52-kept": 320, "all-kept": 320, "all-dropped": 256}[name]


@pytest.mark.parametrize("N,mode", [(640, 0), (1280, 4)])
def test_launches_the_adaptive_kernel_does_not_take_keep_their_bits(N, mode, narrow_switch):
    """N 640 (256 does not divide it) and a fused tail at N 1280: with the switch on, the bits of the switch-off call."""
    o = ops()
    B, K = 5, 128
    M, keep = B * TOK, MASKS[5][0]
    a, b, bias, _ = operands(M, N, K)
    with routed(tile=5 if mode == 0 else 0, image=1):
        assert not o.dense_plan_adaptive(M, N, K, mode, TOK, TOK)[0]
        outs = []
        for on in (True, False):
            narrow_switch.DENSE_NARROW_DROPPED = on
            r = o.dense_gemm_nt(a, b, mode, bias=bias, tokens=TOK, sample_scale=scale_of(keep), rows_per_sample=TOK)
            outs.append(r if isinstance(r, tuple) else (r,))
    for x, y in zip(*outs):
        assert torch.equal(x.view(torch.int16), y.view(torch.int16))
