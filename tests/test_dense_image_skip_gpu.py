"""octic_dense_gemm_nt_tokens_image on the GPU (csrc/dense_gemm.hip dense_plan_image, dense_nt_image_cls_kernel): a masked launch
that the former call keeps on classic 256-row panels runs on per-image panels of the 256-wide tile, nothing split along K, with its
class-token rows computed by workgroups at the end of the grid.

Reference: the SAME build's unmasked launch forced onto per-image panels with nothing split (OCTIC_ROUTE_DENSE_IMAGE = 1,
OCTIC_ROUTE_DENSE_SPLIT = 1, through ops.dense_gemm_nt without a mask = octic_dense_gemm_nt_tokens): kernels that were there before.
The launch under test never splits along K, so every output element sees the reference's MFMA sequence over K; the class-token
workgroups sum slices of 320 in slice order as dense_cls_kernel with K / 320 waves does.  Everything is torch.equal or a bit
pattern - no tolerance anywhere.  Outputs go through the C ABI into buffers pre-filled with NaN, so an unwritten row shows.

Shapes (tokens = 257): B = 1, 2, 13, 17, 18 (class-token row tiles of 16: below, at 16 + 1, 16 + 2, and a B that is no multiple);
(13, 5120) = 260 and (18, 3840) = 270 tiles are two rounds with a partial last one on 256 CUs, (2, 512) is one round; K = 640 /
1280 / 3840 are 2 / 4 / 12 slices (four and two items per pass of a class-token workgroup, and two slices per wave)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOK = 257
DROP = 0.5
SHAPES = [(1, 512, 640), (2, 512, 640), (13, 5120, 1280), (17, 512, 3840), (18, 3840, 1280)]
MODES = (0, 4, 5)


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


@contextlib.contextmanager
def routed(image=0, split=0):
    L = lib()
    try:
        L.route_override(L.ROUTE_DENSE_IMAGE, image)
        L.route_override(L.ROUTE_DENSE_SPLIT, split)
        yield
    finally:
        L.route_override(L.ROUTE_DENSE_IMAGE, 0)
        L.route_override(L.ROUTE_DENSE_SPLIT, 0)


def masks(B):
    """all kept, all dropped, only the first kept, only the last kept, alternating, three seeded Bernoulli(0.5) draws"""
    out = [[1] * B, [0] * B, [1] + [0] * (B - 1), [0] * (B - 1) + [1], [(b + 1) % 2 for b in range(B)]]
    g = torch.Generator().manual_seed(1000 + B)
    out += [(torch.rand(B, generator=g) < 0.5).int().tolist() for _ in range(3)]
    return out


def scale_of(keep):
    return torch.tensor([2.0 if k else 0.0 for k in keep], dtype=torch.float32, device=DEV)


_OPERANDS = {}


def operands(B, N, K):
    """Random bf16 operands of one shape, shared by the cases of that shape and never modified."""
    key = (B, N, K)
    if key not in _OPERANDS:
        if len(_OPERANDS) > 2:
            _OPERANDS.clear()
        M = B * TOK
        g = torch.Generator(device=DEV).manual_seed(104729 * B + 31 * N + K)
        a = torch.randn(M, K, generator=g, device=DEV).to(torch.bfloat16)
        b = (torch.randn(N, K, generator=g, device=DEV) * K ** -0.5).to(torch.bfloat16)
        bias = torch.randn(N, generator=g, device=DEV)
        h = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
        _OPERANDS[key] = (a, b, bias, h)
    return _OPERANDS[key]


_REFERENCE = {}


def reference(B, N, K, mode, a=None):
    """The unmasked per-image launch with nothing split: (C, C2 | column sums | nothing).  `a`: other A rows (mode 5's contract)."""
    key = (B, N, K, mode)
    if a is None and key in _REFERENCE:
        return _REFERENCE[key]
    o = ops()
    a0, b, bias, h = operands(B, N, K)
    with routed(image=1, split=1):
        assert o.dense_plan(B * TOK, N, K, mode, TOK)[2], "the reference is not on per-image panels"
        if mode == 5:
            want = tuple(o.dense_gemm_nt(a0 if a is None else a, b, 5, h=h, want_colsum=True, tokens=TOK))
        else:
            out = o.dense_gemm_nt(a0 if a is None else a, b, mode, bias=bias, tokens=TOK)
            want = tuple(out) if isinstance(out, tuple) else (out,)
    if a is None:
        if len(_REFERENCE) > 6:
            _REFERENCE.clear()
        _REFERENCE[key] = want
    return want


def raw(entry, a, b, bias, h, mode, keep, extra, slab_rows):
    """One launch through the C ABI into NaN-filled outputs -> (C, C2 | finished column sums)."""
    o, L = ops(), lib()
    M, K = a.shape
    N = b.shape[0]
    nan = lambda: torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    c, c2 = nan(), nan() if mode == 4 else None
    cs = torch.full((slab_rows, N), float("nan"), device=DEV) if mode == 5 else None
    P = o._p
    L.check(getattr(L.lib(), entry)(
        P(a), P(b), M, N, K, K, K, mode, P(c), P(c2), N, P(bias) if mode != 5 else None, None, None, 1, None, None,
        P(h) if mode == 5 else None, P(cs), P(scale_of(keep)), TOK, P(o._dense_ws(M, N, K, a.device)), TOK, *extra, o._stream(a)))
    if mode == 4:
        return c, c2
    if mode == 5:
        colsum = torch.empty(N, dtype=torch.float32, device=DEV)
        o._finish(cs, slab_rows, N // 2, colsum, None, None, o._stream(a), out1_ptr=colsum.data_ptr() + 2 * N)
        return c, colsum
    return (c,)


def image_launch(B, N, K, mode, keep, apart=False, a=None):
    """The launch under test, per-image panels forced (these shapes are too small for the model to choose them), class-token rows
    folded or (apart) in their launch; asserts through the plan query which of the two it is."""
    o, L = ops(), lib()
    a0, b, bias, h = operands(B, N, K)
    with routed(image=L.DENSE_IMAGE_ALWAYS + (L.DENSE_IMAGE_CLS_APART if apart else 0)):
        taken, grid, wgs, per_wg, tile_wgs, width, slab_rows, image = o.dense_plan_image(B * TOK, N, K, mode, TOK, TOK, DROP)
        assert taken and image and width == 256 and tile_wgs == B * (N // 256) and slab_rows == 2 * B + (B + 15) // 16
        assert (wgs == 0 and grid == tile_wgs) if apart else (wgs > 0 and grid == tile_wgs + wgs)
        return raw("octic_dense_gemm_nt_tokens_image", a0 if a is None else a, b, bias, h, mode, keep, (0, DROP), slab_rows)


def is_plus_zero(t):
    return bool((t.contiguous().view(torch.int16) == 0).all())


def check_outputs(got, want, B, N, keep, what):
    """Kept samples: every row (class-token row included) equal.  Dropped samples: the class-token row is computed; the patch rows
    are, column tile by column tile, the reference or +0.  No NaN left anywhere."""
    for i, (g, w) in enumerate(zip(got, want)):
        g3, w3 = g.view(B, TOK, N), w.view(B, TOK, N)
        assert not bool(torch.isnan(g.float()).any()), f"{what}: output {i} has an unwritten (or NaN) element"
        kept = torch.tensor(keep, dtype=torch.bool, device=DEV)
        assert torch.equal(g3[kept], w3[kept]), f"{what}: output {i}: rows of kept samples differ"
        assert torch.equal(g3[:, 0], w3[:, 0]), f"{what}: output {i}: class-token rows differ"
        for bi in (bi for bi in range(B) if not keep[bi]):
            for n0 in range(0, N, 256):
                blk, ref = g3[bi, 1:, n0:n0 + 256], w3[bi, 1:, n0:n0 + 256]
                assert is_plus_zero(blk) or torch.equal(blk, ref), f"{what}: output {i}: sample {bi} tile {n0 // 256}"


@pytest.mark.parametrize("mode", (0, 4))
@pytest.mark.parametrize("B,N,K", SHAPES)
def test_forward_modes_every_mask_folded_and_apart(B, N, K, mode):
    want = reference(B, N, K, mode)
    for keep in masks(B):
        folded = image_launch(B, N, K, mode, keep)
        check_outputs(folded, want, B, N, keep, f"mask {keep}")
        apart = image_launch(B, N, K, mode, keep, apart=True)
        for f, s in zip(folded, apart):
            assert torch.equal(f, s), f"mask {keep}: folded and separate class-token routes differ"


@pytest.mark.parametrize("B,N,K", SHAPES)
def test_mode5_zero_rows_of_dropped_samples_give_the_reference_and_its_column_sums(B, N, K):
    """The backward contract: the A rows of a dropped sample are zero.  C equals the reference on kept samples and is a zero on
    the others; the finished column sums are equal (== : up to the sign of an exact zero)."""
    a, b, bias, h = operands(B, N, K)
    for keep in masks(B):
        rowkeep = scale_of(keep).ne(0).repeat_interleave(TOK)
        a0 = a * rowkeep[:, None].to(a.dtype)
        want = reference(B, N, K, 5, a=a0)
        folded = image_launch(B, N, K, 5, keep, a=a0)
        check_outputs(folded[:1], want[:1], B, N, keep, f"mask {keep}")
        assert bool((folded[0].view(B, TOK, N)[~torch.tensor(keep, dtype=torch.bool, device=DEV)] == 0).all())
        assert torch.equal(folded[1], want[1]), f"mask {keep}: column sums differ"
        apart = image_launch(B, N, K, 5, keep, apart=True, a=a0)
        assert torch.equal(folded[0], apart[0]) and torch.equal(folded[1], apart[1]), f"mask {keep}: folded / separate differ"
    assert bool(reference(B, N, K, 5)[1].abs().sum() > 0)


@pytest.mark.parametrize("mode", MODES)
def test_mode5_and_others_with_random_rows_of_dropped_samples(mode):
    """Rows of a dropped sample hold anything (NaN here): no kept row and no class-token sum of a kept sample sees them."""
    B, N, K = 13, 5120, 1280
    a, b, bias, h = operands(B, N, K)
    keep = masks(B)[5]
    assert 0 < sum(keep) < B
    want = reference(B, N, K, mode)
    ap = a.clone()
    drop_rows = (~scale_of(keep).ne(0)).repeat_interleave(TOK)
    patch = torch.arange(B * TOK, device=DEV) % TOK != 0
    ap[drop_rows & patch] = float("nan")                      # (class-token rows are computed for every sample: they stay finite)
    got = image_launch(B, N, K, mode, keep, a=ap)
    kept = torch.tensor(keep, dtype=torch.bool, device=DEV)
    for g, w in zip(got[:2 if mode == 4 else 1], want):
        assert torch.equal(g.view(B, TOK, N)[kept], w.view(B, TOK, N)[kept])
        assert is_plus_zero(g.view(B, TOK, N)[~kept][:, 1:])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,K", [(13, 5120, 1280), (18, 3840, 1280)])
def test_switch_off_and_no_hint_are_the_former_call(B, N, K, mode, monkeypatch):
    """drop = 0 through the new entry, and ops.dense_gemm_nt with functional.DENSE_IMAGE_DROPPED off, are
    octic_dense_gemm_nt_tokens_adaptive bit for bit (here: classic panels with a split-K front)."""
    import octic_vits_amd.functional as OF
    o = ops()
    a, b, bias, h = operands(B, N, K)
    keep = masks(B)[4]
    M = B * TOK
    assert not o.dense_plan_image(M, N, K, mode, TOK, TOK, 0.0)[0] and not o.dense_plan_image(M, N, K, mode, TOK, TOK, DROP, masked=False)[0]
    rows = o.dense_plan(M, N, K, mode, TOK)[1]
    assert o.dense_plan_image(M, N, K, mode, TOK, TOK, 0.0)[5:7] == o.dense_plan(M, N, K, mode, TOK)[:2]
    former = raw("octic_dense_gemm_nt_tokens_adaptive", a, b, bias, h, mode, keep, (), rows)
    nohint = raw("octic_dense_gemm_nt_tokens_image", a, b, bias, h, mode, keep, (0, 0.0), rows)
    monkeypatch.setattr(OF, "DENSE_IMAGE_DROPPED", False)
    kw = dict(tokens=TOK, sample_scale=scale_of(keep), rows_per_sample=TOK, drop=DROP)
    off = o.dense_gemm_nt(a, b, 5, h=h, want_colsum=True, **kw) if mode == 5 else o.dense_gemm_nt(a, b, mode, bias=bias, **kw)
    off = tuple(off) if isinstance(off, tuple) else (off,)
    # (bit patterns: rows that only dead classic panels cover are +0 in all three, the rest are computed)
    for f, n, s in zip(former, nohint, off):
        assert torch.equal(f.view(torch.int16) if f.dtype == torch.bfloat16 else f, n.view(torch.int16) if n.dtype == torch.bfloat16 else n)
        assert torch.equal(f, s)


def test_ops_takes_the_plan_in_force_at_the_headline_shapes():
    """ops.dense_gemm_nt with the drop hint at B = 64: the three multi-round launches go per-image by the model (no knob), the
    column sums come from the slab rows of the plan in force, and kept rows are the reference's."""
    o = ops()
    B, N, K = 64, 5120, 1280
    M = B * TOK
    plan = o.dense_plan_image(M, N, K, 5, TOK, TOK, DROP)
    assert plan[0] and plan[2] > 0 and plan[6] == 2 * B + 4
    a, b, bias, h = operands(B, N, K)
    keep = masks(B)[6]
    a0 = a * scale_of(keep).ne(0).repeat_interleave(TOK)[:, None].to(a.dtype)
    want = reference(B, N, K, 5, a=a0)
    got = o.dense_gemm_nt(a0, b, 5, h=h, want_colsum=True, tokens=TOK, sample_scale=scale_of(keep), rows_per_sample=TOK, drop=DROP)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
