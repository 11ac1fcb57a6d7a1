"""octic_dense_gemm_nt_tokens_adaptive_cls on the GPU (csrc/dense_gemm.hip dense_nt_adaptive_cls_kernel): the adaptive launch
with its class-token rows computed by workgroups at the end of the grid.  A class-token item keeps the arithmetic of the
stand-alone class-token kernels (slices of 320 as ten MFMAs from a zero accumulator, f32 partial tiles summed in slice order,
bias in f32, one rounding), so everything here is bit patterns on random bf16 operands with a bias: the WHOLE output against
octic_dense_gemm_nt_tokens_adaptive of the same build (class-token rows from the stand-alone kernels there, dropped panels +0 in
both), and the class-token rows against the forced single-launch kernel (K 1280) and the forced two-launch path (K 5120).
No tolerance anywhere.

Per-image panels and the 320-wide plan are forced for the small batches (the launch model takes neither that small); every case
asserts through octic_dense_gemm_plan_adaptive_cls that the folded kernel takes the launch, so no case passes on the other path."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOK = 257
N = 1280

MASKS = {
    1: [[1], [0]],
    3: [[1, 0, 1]],
    17: [[1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1]],
}


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


@contextlib.contextmanager
def routed(tile=0, image=0, cls2=0):
    """image = 1 (small batches) also keeps the plan from splitting along K, which it would at K = 5120 on so few tiles."""
    L = lib()
    try:
        L.route_override(L.ROUTE_DENSE_TILE, tile)
        L.route_override(L.ROUTE_DENSE_IMAGE, image)
        L.route_override(L.ROUTE_DENSE_SPLIT, 1 if image == 1 else 0)
        L.route_override(L.ROUTE_DENSE_CLS2, cls2)
        yield
    finally:
        L.route_override(L.ROUTE_DENSE_TILE, 0)
        L.route_override(L.ROUTE_DENSE_IMAGE, 0)
        L.route_override(L.ROUTE_DENSE_SPLIT, 0)
        L.route_override(L.ROUTE_DENSE_CLS2, 0)


@pytest.fixture
def switches():
    import octic_vits_amd.functional as OF
    before = OF.DENSE_NARROW_DROPPED, OF.DENSE_CLS_FOLD
    OF.DENSE_NARROW_DROPPED, OF.DENSE_CLS_FOLD = True, True
    yield OF
    OF.DENSE_NARROW_DROPPED, OF.DENSE_CLS_FOLD = before


_OPERANDS = {}


def operands(M, K):
    """Random bf16 operands and an f32 bias of one shape, shared by the cases of that shape and never modified."""
    key = (M, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 3:
            _OPERANDS.clear()
        g = torch.Generator(device=DEV).manual_seed(7919 * M + K)
        a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        b = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=DEV)
        _OPERANDS[key] = (a, b, bias)
    return _OPERANDS[key]


def scale_of(keep):
    return torch.tensor([2.0 if k else 0.0 for k in keep], dtype=torch.float32, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int16)


def forces():
    L = lib()
    return {"rule": 0, "wide": L.DENSE_ADAPT_WIDE, "narrow": L.DENSE_ADAPT_NARROW}


def check_case(B, K, keep, force, tile=5, image=1):
    """Folded against adaptive, whole output; then the class-token rows against the forced stand-alone path of that K."""
    o = ops()
    M = B * TOK
    a, b, bias = operands(M, K)
    ss = scale_of(keep)
    with routed(tile=tile + force if tile else force, image=image):
        taken, grid, wgs, per_wg, tile_wgs = o.dense_plan_adaptive_cls(M, N, K, 0, TOK, TOK)
        assert taken and tile_wgs == 5 * B == o.dense_plan_adaptive(M, N, K, 0, TOK, TOK)[1] and grid == tile_wgs + wgs and wgs > 0
        want = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=ss, rows_per_sample=TOK)
        got = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=ss, rows_per_sample=TOK, fold_cls=True)
    assert torch.equal(bits(got), bits(want)), "the folded launch differs from the adaptive launch + class-token launches"
    assert bool(torch.isfinite(got.float()).all())
    cls2 = {1280: 1, 5120: 2}.get(K)
    if cls2:
        # (1 = never two launches: dense_cls_kernel<0> with K / 320 waves; 2 = two launches wherever legal)
        with routed(tile=tile + force if tile else force, image=image, cls2=cls2):
            ref = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=ss, rows_per_sample=TOK)
        assert torch.equal(bits(got[::TOK]), bits(ref[::TOK])), "class-token rows differ from the forced stand-alone path"
    return got


@pytest.mark.parametrize("force", ("rule", "wide", "narrow"))
@pytest.mark.parametrize("K", (640, 1280))
@pytest.mark.parametrize("B", (1, 3, 17))
def test_small_batches_equal_the_adaptive_launch(B, K, force, switches):
    """Four / two items per pass of a class-token workgroup; B = 17 has a second, mostly empty row tile (rows past the batch)."""
    for keep in MASKS[B]:
        check_case(B, K, keep, forces()[force])


@pytest.mark.parametrize("force", ("rule", "wide", "narrow"))
def test_two_slices_per_wave_at_k_5120(force, switches):
    """16 slices: wave w contracts slices w and w + 8 into separate partial tiles."""
    check_case(3, 5120, MASKS[3][0], forces()[force])


KEPT = {"38-kept": 38, "39-kept": 39, "51-kept": 51, "52-kept": 52, "all-kept": 64, "none-kept": 0}


@pytest.mark.parametrize("force", ("rule", "wide", "narrow"))
@pytest.mark.parametrize("name", list(KEPT))
def test_kept_counts_at_64_images(name, force, switches):
    """B 64, K 640 - the plan the model chooses by itself: 64 or more CUs free up to 38 kept, the narrow tile up to 51, every CU
    on a live tile with all kept (the class-token workgroups then run behind the tiles)."""
    n = KEPT[name]
    keep = [1] * n + [0] * (64 - n)
    keep = [keep[(b * 37) % 64] for b in range(64)]                  # a fixed permutation (37 is coprime to 64)
    assert sum(keep) == n
    got = check_case(64, 640, keep, forces()[force], tile=0, image=0)
    if n == 0:
        patches = torch.ones(64 * TOK, dtype=torch.bool, device=DEV)
        patches[::TOK] = False
        assert bool((bits(got[patches]) == 0).all())                 # every panel dead: +0 ...
        assert bool((got[::TOK].float().abs() > 0).any())            # ... and the class-token rows computed all the same


def test_every_row_is_written_with_a_wide_output(switches):
    """ldc > N and a NaN-filled output buffer: every row of [M, N] is written (class-token rows of dropped samples too), nothing
    beyond column N is touched, and the bits are the adaptive launch's in the same buffer geometry."""
    o, L = ops(), lib()
    B, K, ldc = 17, 1280, N + 64
    M, keep = B * TOK, MASKS[17][0]
    a, b, bias = operands(M, K)
    ss = scale_of(keep)
    ws = o._dense_ws(M, N, K, a.device)
    outs = []
    with routed(tile=5, image=1):
        assert o.dense_plan_adaptive_cls(M, N, K, 0, TOK, TOK)[0]
        for fold in (1, 0):
            c = torch.full((M, ldc), float("nan"), dtype=torch.bfloat16, device=DEV)
            o.check(L.lib().octic_dense_gemm_nt_tokens_adaptive_cls(
                o._p(a), o._p(b), M, N, K, a.stride(0), b.stride(0), 0, o._p(c), None, ldc, o._p(bias), None, None, 1, None, None,
                None, None, o._p(ss), TOK, o._p(ws), TOK, fold, o._stream(a)))
            outs.append(c)
    got, want = outs
    assert not bool(torch.isnan(got[:, :N].float()).any()), "a row of the output was not written"
    assert bool(torch.isnan(got[:, N:].float()).all()), "the launch wrote past column N"
    assert torch.equal(bits(got[:, :N]), bits(want[:, :N]))


def test_a_k_the_fold_does_not_take_equals_the_adaptive_call(switches):
    """K 256 is no multiple of 320: with fold_cls the call IS octic_dense_gemm_nt_tokens_adaptive."""
    o = ops()
    B, K = 3, 256
    M, keep = B * TOK, MASKS[3][0]
    a, b, bias = operands(M, K)
    ss = scale_of(keep)
    with routed(tile=5, image=1):
        assert o.dense_plan_adaptive(M, N, K, 0, TOK, TOK)[0] and not o.dense_plan_adaptive_cls(M, N, K, 0, TOK, TOK)[0]
        want = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=ss, rows_per_sample=TOK)
        got = o.dense_gemm_nt(a, b, 0, bias=bias, tokens=TOK, sample_scale=ss, rows_per_sample=TOK, fold_cls=True)
    assert torch.equal(bits(got), bits(want))
