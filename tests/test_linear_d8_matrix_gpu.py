"""The LinearD8 GEMM family - forward and input gradient (csrc/gemm.hip linear_d8_kernel<TIN, TOUT, NT> and
linear_d8_ring_kernel, csrc/gemm_wreg.hip linear_d8_wreg_kernel), weight gradient (csrc/wgrad.hip wgrad_kernel<TIN, TT>,
wgrad_ring_kernel, wgrad_finish_kernel), octic_linear_d8_prep and octic_colsum_a1 - on operands whose products and partial
sums are EXACT in f32 in any summation order.  Every comparison is bit for bit against float64 (`!=`, so +0 equals -0):
one dropped or doubled K element, a wrong row of a split, a wrong column of a tile is a wrong number, not noise.  There is no
tolerance in this file.

Operands (seeded from the shape)
  forward: x integers in [-3, 3].  Irrep group g has K_g = cin (A1, A2, B1, B2) or 2 cin (E); W_g = integers in [-2, 2] times
    2^-s_g, s_g = round(0.5 log2(8 K_g)) (unit-scale outputs); bias in quarters within [-1, 1]; cs (per channel) from
    {+-0.5, +-1, +-2}; rs (per sample) in {0, 2}, samples 0 and 1 forced to 0 and 2 (a launch of ONE sample gets 2, so its GEMM
    result still shows); resid integers in [-8, 8] in the output dtype.  All of it is exact in bf16 and in f32; |acc| 2^s is
    an integer <= 6 K < 2^24 and the scales are powers of two, so resid + rs cs (acc + bias) is an exactly known f32 value
    whatever the summation or epilogue order and whether the bias enters before or after the K loop.  The generator asserts
    6 K < 2^24 and, in float64, that the accumulator and the pre-rounding output survive an f32 round trip.  Reference: the
    formula of include/octic_hip.h (octic_linear_d8_fwd) in torch float64, E as [M, 2, 2 cin] @ W_E^T; f32 outputs bit for
    bit, bf16 outputs bit for bit after the ONE f32 -> bf16 rounding of the known value.
  weight gradient: dy integers in [-2, 2], x as above: every partial and total sum G is an integer <= 6 rows; master weights
    and cs as above; dW = cs G, dbias = cs_A1 dysum and dcs = <W, G> + bias dysum are exact while 12 rows_E K_E < 2^24
    (asserted per case; the largest here is 12 * 402 * 368 < 2^21).  x and dy carry 64 rows of non-zero values behind row M
    (the tile kernels stage 64 | 32 reduction rows at a time): a row guard that let them in is a wrong number.
  input gradient: dy integers in [-2, 2] against wt_g[k][n] = cs_g[n] W_g[n][k] from octic_linear_d8_prep (exact: cs is a power
    of two); |acc| 2^(s+1) is an integer <= 16 N.

Guards: every output is prefilled with a sentinel (NaN for f32, the bf16 bit pattern 0x5A5B) and has one guard row in front
and one behind; after the launch every cell of the output is written and every guard cell holds the sentinel, as do the
padding columns of the strided layout and the region behind octic_linear_d8_wgrad_workspace_bytes.

Every case asserts the kernel it is about to run (kernel id, tile width, fused flag) through _lib.plan before it launches;
test_the_tables_reach_every_branch checks the tables below against the routing rules without a GPU.

Shapes.  M in {1, 201} with rows_per_sample 1 and 67: the one-dimensional groups have 2 row tiles with a 73-row tail, E has
402 rows = 4 row tiles with an 18-row tail and odd / even pair addressing.
  1. register-staged kernel (linear_d8_kernel): bf16 cin = every multiple of 8 up to 184 that is not a multiple of 32 (K
     remainders 8 .. 56 after 0, 1, 2 full K tiles of 64; E: 1 .. 6 K tiles, remainders 16 / 32 / 48 - 32 is the
     last_half_only edge k_rem == 4 EPC), cout 8 / 40 / 104 / 136 = tile 64 / 96 / 128 / 160, each with a column tail, E's
     2 cout a second, partial column tile for the last two; f32 cin = every multiple of 4 up to 124 that is not a multiple
     of 16 (remainders 4 .. 28 after 0 .. 3 full K tiles of 32; E 1 .. 8 K tiles, remainders 8 / 16 / 24), cout 4 / 36 / 100
     / 132.  Plain with bias and fused with bias + resid + rs + cs; once per tile width and dtype pair from five separate
     tensors whose row strides are 8 elements wider than their rows (ops.tview).
  2. bf16 cin 32 .. 160 as routed (W-stationary kernel) and under OCTIC_ROUTE_LINEAR_RING = 1 (ring, tile 80); bf16 cin 192 / 320
     (ring, tile 80; (320, 160) is the wide tile); (320, 160) and (640, 160) (ring, tile 160); f32 cin 16 / 48 / 80 / 160 / 176
     (ring, tile 80); cout 8 / 40 / 104 / 160.
  3. octic_linear_d8_prep + the input gradient at ViT-S (48, 144), (48, 48), (48, 192), (192, 48), ViT-Ti (24, 72), (24, 96)
     and (104, 40), (160, 480): bf16 cin' = 144 on the register-staged kernel, 192-wide ring shapes, 480 -> 160 on the wide ring.
  4. wgrad_kernel<TIN, TT>: tile 64 (8, 8), (24, 72), (184, 8) [3 and 6 K tiles, a 56-wide tail], (124, 132) [f32: 2 x 3 tiles];
     tile 96 (48, 144), (72, 72); tile 128 (104, 104); tile 160 (136, 136); wgrad_ring_kernel (bf16) (160, 160), (160, 480).
     splits in {1, 2, 3, 8, 9, 32} through the C ABI: 32 leaves most row splits of 201 rows empty (they must contribute exact
     zeros), 8 and 9 cross the 8-way unrolled slab sum of wgrad_finish_body.  Finish without cs, with cs + w32 + bias + an
     explicit dysum from ops.colsum_a1, and on ring shapes with dysum = NULL (the kernel's own column sums)."""
import contextlib
import ctypes
import math

import pytest
import torch

from test_gemm_plan_host import linear_expected, wgrad_expected          # the routing rules: import without the built library

gpu = pytest.mark.gpu

DEV = "cuda"
bf, f32 = torch.bfloat16, torch.float32
SENTINEL = 0x5A5B                                   # bf16 bit pattern of the guard cells
WREG, RING, CLASSIC = range(3)                      # OCTIC_LINEAR_*
WG_RING, WG_TILED = range(2)                        # OCTIC_WGRAD_*
NAMES = ("A1", "A2", "B1", "B2", "E")
PAIRS = {"f32": (f32, f32), "bf16": (bf, bf), "bf16-f32": (bf, f32)}
ROWS = ((1, 1), (201, 67))                          # (M, rows_per_sample)
TAIL = 64                                           # non-zero rows behind the weight gradient's operands
WS_GUARD = 4096                                     # floats behind the weight gradient's workspace

# ---- 1. register-staged kernel: cout -> tile, per operand dtype
CLASSIC_TILE = {bf: {8: 64, 40: 96, 104: 128, 136: 160}, f32: {4: 64, 36: 96, 100: 128, 132: 160}}
STRIDED_CIN = {bf: 88, f32: 44}                     # one full K tile + a 24 | 12 remainder; E two full + 48 | 24

# ---- 2. (family, operand dtype) -> (cins, couts, knob, kernel)
RING_COUTS = (8, 40, 104, 160)
FAMILIES = {
    "wreg": (bf, (32, 64, 96, 128, 160), RING_COUTS, 0, WREG),
    "ring-knob": (bf, (32, 64, 96, 128, 160), RING_COUTS, 1, RING),
    "ring": (bf, (192, 320), RING_COUTS, 0, RING),
    "ring-wide": (bf, (320, 640), (160,), 0, RING),
    "ring-f32": (f32, (16, 48, 80, 160, 176), RING_COUTS, 0, RING),
}
WIDE = ((320, 160), (640, 160))                     # bf16 ring shapes on the 160-column tile

# ---- 3. (cin, cout) -> {operand dtype: ((forward kernel, tile), (input-gradient kernel, tile))}
PREP = {
    (48, 144): {bf: ((CLASSIC, 160), (CLASSIC, 96)), f32: ((RING, 80), (RING, 80))},
    (48, 48): {bf: ((CLASSIC, 96), (CLASSIC, 96)), f32: ((RING, 80), (RING, 80))},
    (48, 192): {bf: ((CLASSIC, 96), (RING, 80)), f32: ((RING, 80), (RING, 80))},
    (192, 48): {bf: ((RING, 80), (CLASSIC, 96)), f32: ((RING, 80), (RING, 80))},
    (24, 72): {bf: ((CLASSIC, 96), (CLASSIC, 64)), f32: ((CLASSIC, 96), (CLASSIC, 64))},
    (24, 96): {bf: ((CLASSIC, 96), (WREG, 0)), f32: ((CLASSIC, 96), (RING, 80))},
    (104, 40): {bf: ((CLASSIC, 96), (CLASSIC, 128)), f32: ((CLASSIC, 96), (CLASSIC, 128))},
    (160, 480): {bf: ((WREG, 0), (RING, 160)), f32: ((RING, 80), (RING, 80))},
}

# ---- 4. (cin, cout) -> (tile, operand dtypes); bf16 on (160, *160) is the ring kernel
WGRAD = {(8, 8): (64, (f32, bf)), (24, 72): (64, (f32, bf)), (184, 8): (64, (f32, bf)), (124, 132): (64, (f32,)),
         (48, 144): (96, (f32, bf)), (72, 72): (96, (f32, bf)), (104, 104): (128, (f32, bf)), (136, 136): (160, (f32, bf)),
         (160, 160): (160, (f32, bf)), (160, 480): (160, (f32, bf))}
SPLITS = (1, 2, 3, 8, 9, 32)


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


def code(dtype):
    return 0 if dtype == f32 else 1                 # OCTIC_F32 | OCTIC_BF16


def classic_cins(dtype):
    """The widths of section 1: every legal width up to 184 | 124 that no ring or W-stationary kernel takes."""
    step, top, ring = (8, 184, 32) if dtype == bf else (4, 124, 16)
    return [c for c in range(step, top + 1, step) if c % ring]


# ---- the exact problems ----------------------------------------------------------------------------------------------
class Problem:
    pass


def shapes5(M, c):
    return [(M, c)] * 4 + [(M, 2, 2 * c)]


def shift(K):
    return round(0.5 * math.log2(8.0 * K))


def f32_exact(t, what):
    assert torch.equal(t.float().double(), t), f"{what} is not an f32 value: the operand ranges are too wide for this shape"


def generator(tag, *dims):
    seed = tag
    for d in dims:
        seed = seed * 1000003 + d
    g = torch.Generator(device=DEV).manual_seed(seed % (2 ** 62))
    return lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=DEV).double()


def weights(ri, cin, cout):
    w5 = [ri(-2, 2, cout, cin) * 2.0 ** -shift(cin) for _ in range(4)] + [ri(-2, 2, 2 * cout, 2 * cin) * 2.0 ** -shift(2 * cin)]
    for w, K in zip(w5, (cin,) * 4 + (2 * cin,)):
        assert 6 * K < 2 ** 24 and float((w * 2.0 ** shift(K)).frac().abs().max()) == 0
    return w5


def scales(ri, cout):
    table = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=torch.float64, device=DEV)
    return [table[ri(0, 5, cout if i < 4 else 2 * cout).long()] for i in range(5)]


def linear64(x5, w5, bias=None, resid5=None, rsrow=None, cs5=None):
    """resid + rs cs (x W^T + bias on A1) per irrep in float64 (octic_linear_d8_fwd of include/octic_hip.h)."""
    ys = []
    for i in range(5):
        y = x5[i] @ w5[i].t()
        if i == 0 and bias is not None:
            y = y + bias
        if cs5 is not None:
            y = y * cs5[i]
        if rsrow is not None:
            y = y * rsrow.reshape((-1,) + (1,) * (y.dim() - 1))
        if resid5 is not None:
            y = y + resid5[i]
        ys.append(y)
    return ys


_LAST = {}


def forward_problem(M, rps, cin, cout):
    """Exact operands and the float64 results of one forward shape (kept for the launches of that shape that follow)."""
    key = ("fwd", M, rps, cin, cout)
    if _LAST.get("key") == key:
        return _LAST["p"]
    _LAST.clear()
    ri = generator(1, M, cin, cout)
    p = Problem()
    p.M, p.rps, p.cin, p.cout = M, rps, cin, cout
    p.x5 = [ri(-3, 3, *s) for s in shapes5(M, cin)]
    p.w5 = weights(ri, cin, cout)
    p.bias = ri(-4, 4, cout) / 4
    p.cs5 = scales(ri, cout)
    ns = -(-M // rps)
    p.rs = 2.0 * ri(0, 1, ns)
    if ns > 1:
        p.rs[0], p.rs[1] = 0.0, 2.0
    else:
        p.rs[0] = 2.0
    p.resid5 = [ri(-8, 8, *s) for s in shapes5(M, cout)]
    for acc in linear64(p.x5, p.w5):
        f32_exact(acc, "an accumulator")
    p.plain5 = linear64(p.x5, p.w5, p.bias)
    p.fused5 = linear64(p.x5, p.w5, p.bias, p.resid5, p.rs.repeat_interleave(rps)[:M], p.cs5)
    for y in p.plain5 + p.fused5:
        f32_exact(y, "an output before its rounding")
    _LAST["key"], _LAST["p"] = key, p
    return p


def pack5(t5, dtype):
    """The five tensors as one packed [rows, 8c] = [A1|A2|B1|B2|E_row0|E_row1] in `dtype`."""
    return torch.cat([t5[0], t5[1], t5[2], t5[3], t5[4].flatten(-2)], dim=-1).to(dtype).contiguous()


# ---- sentinels and comparisons -----------------------------------------------------------------------------------------
def sentinel(shape, dtype):
    if dtype == f32:
        return torch.full(shape, float("nan"), dtype=f32, device=DEV)
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(bf)


def is_sentinel(t):
    return t.isnan() if t.dtype == f32 else t.view(torch.int16) == SENTINEL


def untouched(t, what):
    assert bool(is_sentinel(t).all()), f"{what}: {int((~is_sentinel(t)).sum())} guard cells were written"


def written(t, what):
    assert not bool(is_sentinel(t).any()), f"{what}: {int(is_sentinel(t).sum())} of {t.numel()} cells were not written"


def exact(got, want, what):
    got, want = (t.reshape(1, -1) if t.dim() == 1 else t.reshape(-1, t.shape[-1]) for t in (got, want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()
        rows, cols = idx[:, 0], idx[:, 1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements wrong, rows {int(rows.min())}..{int(rows.max())}, "
                             f"columns {int(cols.min())}..{int(cols.max())}; first {idx[0].tolist()} got {float(got[tuple(idx[0])])} "
                             f"want {float(want[tuple(idx[0])])}")


def rounded(t64, dtype):
    """The ONE rounding of an exactly known f32 value."""
    return t64.float().to(dtype)


def exact5(got5, want5, dtype, what):
    """Per irrep; E is compared as its [2M, 2c] GEMM rows (row 2m + e)."""
    for i in range(5):
        written(got5[i], f"{what}, irrep {NAMES[i]}")
        exact(got5[i], rounded(want5[i], dtype), f"{what}, irrep {NAMES[i]}")


def unpack(y, c):
    return [y[:, i * c:(i + 1) * c] for i in range(4)] + [y[:, 4 * c:].reshape(-1, 2 * c)]


# ---- plans ---------------------------------------------------------------------------------------------------------------
def linear_plan_is(M, cin, cout, dt, odt, fused, kernel, tile):
    got = lib().plan("octic_linear_d8_plan", M, cin, cout, code(dt), code(odt), int(fused))
    want = (kernel, tile, 0 if kernel == CLASSIC else int(fused), 0)
    assert got == want, f"M {M}, {cin} -> {cout}, fused {fused}: the plan is {got}, this case is about {want}"


def wgrad_plan_is(M, cin, cout, dt, kernel, tile):
    got = lib().plan("octic_linear_d8_wgrad_plan", M, cin, cout, code(dt))
    assert got is not None and (got[0], got[1], got[3]) == (kernel, tile, int(kernel == WG_RING)), \
        f"M {M}, {cin} -> {cout}: the weight-gradient plan is {got}, this case is about kernel {kernel}, tile {tile}"


@contextlib.contextmanager
def ring_knob(value):
    """OCTIC_ROUTE_LINEAR_RING for the launches inside; back at 0 afterwards, and checked to be."""
    L = lib()
    try:
        if value:
            assert L.route_override(L.ROUTE_LINEAR_RING, value) == 0
        yield
    finally:
        L.route_override(L.ROUTE_LINEAR_RING, 0)
    assert L.route_override(L.ROUTE_LINEAR_RING, 0) == 0
    assert L.plan("octic_linear_d8_plan", 96, 32, 32, 1, 1, 0) == (WREG, 0, 0, 0), "the ring knob is not back at 0"


# ---- forward launches ----------------------------------------------------------------------------------------------------
def run_packed(o, x5, w5, bias, want5, M, cin, cout, dt, odt, what, resid5=None, rs=None, rps=1, cs5=None):
    """One launch from packed rows into a sentinel-filled output with a guard row on either side."""
    x = pack5(x5, dt)
    ybuf = sentinel((M + 2, 8 * cout), odt)
    y = ybuf[1:M + 1]
    kw = {}
    if resid5 is not None:
        r = pack5(resid5, odt)
        kw = dict(resid_v=o.pview(r, cout), rs=rs.float(), rps=rps, cs5=[c.float() for c in cs5])
    o.linear_fwd(o.pview(x, cin), [w.to(dt).contiguous() for w in w5], None if bias is None else bias.float(), o.pview(y, cout),
                 M, cin, cout, dt, odt, x, **kw)
    torch.cuda.synchronize()
    untouched(ybuf[0], f"{what}: the row in front of the output")
    untouched(ybuf[M + 1], f"{what}: the row behind the output")
    exact5(unpack(y, cout), want5, odt, what)


def run_forward(o, M, rps, cin, cout, dt, odt, fused, kernel, tile):
    p = forward_problem(M, rps, cin, cout)
    linear_plan_is(M, cin, cout, dt, odt, fused, kernel, tile)
    what = f"M {M}, {cin} -> {cout}, {'fused' if fused else 'plain'}"
    if fused:
        run_packed(o, p.x5, p.w5, p.bias, p.fused5, M, cin, cout, dt, odt, what, p.resid5, p.rs, rps, p.cs5)
    else:
        run_packed(o, p.x5, p.w5, p.bias, p.plain5, M, cin, cout, dt, odt, what)


def strided5(M, c, dtype, values5=None, fill=None):
    """Five separate tensors with one guard row on either side and row strides 8 elements wider than the rows: (views, buffers).
    Inputs: `values5` inside, `fill` everywhere else; outputs: the sentinel everywhere."""
    views, bufs = [], []
    for i in range(5):
        width = c if i < 4 else 4 * c
        buf = sentinel((M + 2, width + 8), dtype) if values5 is None else torch.full((M + 2, width + 8), fill, dtype=dtype, device=DEV)
        v = buf[1:M + 1, :width]
        if values5 is not None:
            v.copy_(values5[i].reshape(M, width).to(dtype))
        views.append(v if i < 4 else v.unflatten(-1, (2, 2 * c)))
        bufs.append(buf)
    return views, bufs


def run_strided(o, p, dt, odt, fused, what):
    M, cin, cout = p.M, p.cin, p.cout
    xs, _ = strided5(M, cin, dt, p.x5, 5.0)
    ys, ybufs = strided5(M, cout, odt)
    xv, keep_x = o.tview(xs, cin)
    yv, keep_y = o.tview(ys, cout)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(keep_x + keep_y, xs + ys)), "tview copied a strided tensor"
    assert list(xv.ld) == [cin + 8] * 4 + [4 * cin + 8] and list(yv.ld) == [cout + 8] * 4 + [4 * cout + 8]
    kw = {}
    if fused:
        rsd, _ = strided5(M, cout, odt, p.resid5, 9.0)
        rv, keep_r = o.tview(rsd, cout)
        assert all(a.data_ptr() == b.data_ptr() for a, b in zip(keep_r, rsd))
        kw = dict(resid_v=rv, rs=p.rs.float(), rps=p.rps, cs5=[c.float() for c in p.cs5])
    o.linear_fwd(xv, [w.to(dt).contiguous() for w in p.w5], p.bias.float(), yv, M, cin, cout, dt, odt, xs[0], **kw)
    torch.cuda.synchronize()
    for i, buf in enumerate(ybufs):
        width = cout if i < 4 else 4 * cout
        untouched(buf[0], f"{what}, irrep {NAMES[i]}: the row in front")
        untouched(buf[M + 1], f"{what}, irrep {NAMES[i]}: the row behind")
        untouched(buf[:, width:], f"{what}, irrep {NAMES[i]}: the padding columns")
    exact5(ys, p.fused5 if fused else p.plain5, odt, what)


# ---- the tables, without a GPU ---------------------------------------------------------------------------------------------
def _k_tiles(K, dtype):
    """(K tiles, valid K elements of the last one) of the register-staged kernel: 128-byte tiles."""
    bke = 64 if dtype == bf else 32
    nkt = -(-K // bke)
    return nkt, K - (nkt - 1) * bke


def test_the_tables_reach_every_branch():
    """What the loops of this file visit, against the routing rules (tests/test_gemm_plan_host.py) and the library's plans."""
    L = lib()
    for name, (dt, odt) in PAIRS.items():
        visited = set()
        for cout, tile in CLASSIC_TILE[dt].items():
            for cin in classic_cins(dt):
                for M, _ in ROWS:
                    for fused in (0, 1):
                        want = (CLASSIC, tile, 0, 0)
                        assert linear_expected(M, cin, cout, code(dt), fused) == want, (name, M, cin, cout)
                        assert L.plan("octic_linear_d8_plan", M, cin, cout, code(dt), code(odt), fused) == want, (name, M, cin, cout)
                (nkt, rem), (nkt_e, rem_e) = _k_tiles(cin, dt), _k_tiles(2 * cin, dt)
                visited.add((tile, rem, rem_e, nkt, nkt_e))
        if dt == bf:
            rems, fulls, rems_e, tiles_e, n = (8, 16, 24, 40, 48, 56), (0, 1, 2), (16, 32, 48), range(1, 7), 18
        else:
            rems, fulls, rems_e, tiles_e, n = (4, 8, 12, 20, 24, 28), (0, 1, 2, 3), (8, 16, 24), range(1, 9), 24
        assert len(classic_cins(dt)) == n and len(visited) == 4 * n
        assert {(t, r, k - 1) for t, r, _, k, _ in visited} == {(t, r, f) for t in (64, 96, 128, 160) for r in rems for f in fulls}
        assert {(t, r, k) for t, _, r, _, k in visited} >= {(t, r, 1) for t in (64, 96, 128, 160) for r in rems_e}
        assert {k for _, _, _, _, k in visited} == set(tiles_e) and {r for _, _, r, _, _ in visited} == set(rems_e)
        # a column tail inside every tile; a second, partial column tile of E for the two wide ones
        for cout, tile in CLASSIC_TILE[dt].items():
            assert cout % tile and (2 * cout) % tile and (-(-2 * cout // tile) == 2) == (tile >= 128)
        assert STRIDED_CIN[dt] in classic_cins(dt)
    # section 2: the kernel of every family, with and without the knob (the rules take the knob as an argument)
    for family, (dt, cins, couts, knob, kernel) in FAMILIES.items():
        for cin in cins:
            for cout in couts:
                tile = 0 if kernel == WREG else (160 if dt == bf and (cin, cout) in WIDE else 80)
                for M, _ in ROWS:
                    assert linear_expected(M, cin, cout, code(dt), 1, ring_knob=bool(knob)) == (kernel, tile, 1, 0), (family, cin, cout)
    assert {(cin, cout) for cin in FAMILIES["ring-wide"][1] for cout in FAMILIES["ring-wide"][2]} == set(WIDE)
    # section 3: forward and input gradient (cin and cout swapped) of every pair
    for (cin, cout), per_dtype in PREP.items():
        for dt, (fwd, bwd) in per_dtype.items():
            for M, _ in ROWS:
                assert linear_expected(M, cin, cout, code(dt), 0)[:2] == fwd, (cin, cout, dt)
                assert linear_expected(M, cout, cin, code(dt), 0)[:2] == bwd, (cin, cout, dt)
                assert L.plan("octic_linear_d8_plan", M, cout, cin, code(dt), code(dt), 0)[:2] == bwd
    assert PREP[(48, 144)][bf][1] == (CLASSIC, 96) and PREP[(160, 480)][bf][1] == (RING, 160)
    # section 4
    for (cin, cout), (tile, dtypes) in WGRAD.items():
        for dt in dtypes:
            ring = dt == bf and cin % 160 == 0 and cout % 160 == 0
            for M, _ in ROWS:
                kernel, width, _, has_colsum = wgrad_expected(M, cin, cout, code(dt))
                assert (kernel, width, has_colsum) == (WG_RING if ring else WG_TILED, tile, int(ring)), (cin, cout, dt)
                got = L.plan("octic_linear_d8_wgrad_plan", M, cin, cout, code(dt))
                assert (got[0], got[1], got[3]) == (kernel, width, has_colsum)
            assert 12 * 402 * 2 * cin < 2 ** 24
    assert {t for t, _ in WGRAD.values()} == {64, 96, 128, 160}
    assert -(-184 // 64) == 3 and -(-368 // 64) == 6 and 184 % 64 == 56 and (-(-124 // 64), -(-132 // 64)) == (2, 3)


# ---- 1. the register-staged kernel -------------------------------------------------------------------------------------------
CLASSIC_CASES = [(name, cout) for name, (dt, _) in PAIRS.items() for cout in CLASSIC_TILE[dt]]


@gpu
@pytest.mark.parametrize("fused", (False, True), ids=("plain", "fused"))
@pytest.mark.parametrize("pair,cout", CLASSIC_CASES)
def test_classic_forward(pair, cout, fused):
    """linear_d8_kernel<TIN, TOUT, NT> at every K remainder behind 0 .. 2 (bf16) | 0 .. 3 (f32) full K tiles, M = 1 and 201."""
    o = ops()
    dt, odt = PAIRS[pair]
    for cin in classic_cins(dt):
        for M, rps in ROWS:
            run_forward(o, M, rps, cin, cout, dt, odt, fused, CLASSIC, CLASSIC_TILE[dt][cout])


@gpu
@pytest.mark.parametrize("pair,cout", CLASSIC_CASES)
def test_classic_forward_from_strided_tuple_layout(pair, cout):
    """The same launch from five separate tensors with padded rows (ops.tview): same exact result, padding left alone."""
    o = ops()
    dt, odt = PAIRS[pair]
    M, rps = ROWS[1]
    p = forward_problem(M, rps, STRIDED_CIN[dt], cout)
    for fused in (False, True):
        linear_plan_is(M, p.cin, cout, dt, odt, fused, CLASSIC, CLASSIC_TILE[dt][cout])
        run_strided(o, p, dt, odt, fused, f"strided {p.cin} -> {cout}, {'fused' if fused else 'plain'}")


# ---- 2. ring and W-stationary kernels on the same problems --------------------------------------------------------------------
FAMILY_CASES = [(name, family) for family, spec in FAMILIES.items() for name, (dt, _) in PAIRS.items() if dt == spec[0]]


@gpu
@pytest.mark.parametrize("pair,family", FAMILY_CASES)
def test_ring_and_w_stationary_forward(pair, family):
    o = ops()
    dt, odt = PAIRS[pair]
    _, cins, couts, knob, kernel = FAMILIES[family]
    with ring_knob(knob):
        for cin in cins:
            for cout in couts:
                tile = 0 if kernel == WREG else (160 if dt == bf and (cin, cout) in WIDE else 80)
                for M, rps in ROWS:
                    for fused in (False, True):
                        run_forward(o, M, rps, cin, cout, dt, odt, fused, kernel, tile)


# ---- 3. prepared weights and the input gradient -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", (f32, bf), ids=("f32", "bf16"))
@pytest.mark.parametrize("cin,cout", list(PREP))
def test_prepared_weights_and_input_gradient(cin, cout, dtype):
    """octic_linear_d8_prep: wb = W and wt_g[k][n] = cs_g[n] W_g[n][k] bit for bit; dX = dY diag(cs) W through
    octic_linear_d8_fwd with the transposed weights and cin, cout swapped; the forward with wb on the way."""
    o = ops()
    fwd, bwd = PREP[(cin, cout)][dtype]
    ri = generator(3, cin, cout)
    w5, cs5 = weights(ri, cin, cout), scales(ri, cout)
    wb, wt = o.linear_prep([w.float().contiguous() for w in w5], [c.float() for c in cs5], cin, cout, dtype)
    torch.cuda.synchronize()
    wt64 = [(c[:, None] * w).t() for c, w in zip(cs5, w5)]
    for i in range(5):
        exact(wb[i], w5[i].to(dtype), f"wb {NAMES[i]}")
        exact(wt[i], wt64[i].to(dtype), f"wt {NAMES[i]}")
        assert torch.equal(w5[i].to(dtype).double(), w5[i]) and torch.equal(wt64[i].to(dtype).double(), wt64[i])
    for M, rps in ROWS:
        dy5 = [ri(-2, 2, *s) for s in shapes5(M, cout)]
        x5 = [ri(-3, 3, *s) for s in shapes5(M, cin)]
        dx5 = linear64(dy5, wt64)
        y5 = linear64(x5, w5)
        for t in dx5 + y5:
            f32_exact(t, "an accumulator")
        for odt in ((f32,) if dtype == f32 else (f32, bf)):
            linear_plan_is(M, cout, cin, dtype, odt, False, *bwd)
            run_packed(o, dy5, wt, None, dx5, M, cout, cin, dtype, odt, f"input gradient, M {M}, {cout} -> {cin}")
            linear_plan_is(M, cin, cout, dtype, odt, False, *fwd)
            run_packed(o, x5, wb, None, y5, M, cin, cout, dtype, odt, f"forward with wb, M {M}, {cin} -> {cout}")


# ---- 4. weight gradient ------------------------------------------------------------------------------------------------------
def wgrad_problem(M, cin, cout):
    ri = generator(4, M, cin, cout)
    p = Problem()
    p.M, p.cin, p.cout = M, cin, cout
    p.x5 = [ri(-3, 3, *s) for s in shapes5(M, cin)]
    p.dy5 = [ri(-2, 2, *s) for s in shapes5(M, cout)]
    p.w5, p.cs5, p.bias = weights(ri, cin, cout), scales(ri, cout), ri(-4, 4, cout) / 4
    assert 12 * (2 * M) * (2 * cin) < 2 ** 24
    N5, K5 = (cout,) * 4 + (2 * cout,), (cin,) * 4 + (2 * cin,)
    p.g5 = [p.dy5[i].reshape(-1, N5[i]).t() @ p.x5[i].reshape(-1, K5[i]) for i in range(5)]
    p.dysum = p.dy5[0].sum(0)
    p.dw5 = [p.cs5[i][:, None] * p.g5[i] for i in range(5)]
    p.dcs5 = [(p.w5[i] * p.g5[i]).sum(1) + (p.bias * p.dysum if i == 0 else 0.0) for i in range(5)]
    p.dbias = p.cs5[0] * p.dysum
    for t in p.g5 + p.dw5 + p.dcs5 + [p.dbias, p.dysum]:
        f32_exact(t, "a weight-gradient result")
    return p


def with_tail(t5, dtype, fill):
    """The packed rows as the first M rows of a buffer whose TAIL further rows hold `fill`."""
    rows = pack5(t5, dtype)
    buf = torch.full((rows.shape[0] + TAIL, rows.shape[1]), fill, dtype=dtype, device=DEV)
    buf[:rows.shape[0]] = rows
    return buf[:rows.shape[0]]


def run_finish(o, p, ws, splits, scaled, dysum, what):
    """octic_linear_d8_wgrad_finish into sentinel-filled outputs with a guard row on either side; everything exact."""
    L = lib()
    cin, cout = p.cin, p.cout
    N5, K5 = (cout,) * 4 + (2 * cout,), (cin,) * 4 + (2 * cin,)
    dwb = [sentinel((N5[i] + 2, K5[i]), f32) for i in range(5)]
    dcsb = [sentinel((3, N5[i]), f32) for i in range(5)]
    dbb = sentinel((3, cout), f32)
    dw, dcs, dbias = [b[1:-1] for b in dwb], [b[1] for b in dcsb], dbb[1]
    w32 = [w.float().contiguous() for w in p.w5]
    cs, bias = [c.float() for c in p.cs5], p.bias.float()
    L.check(L.lib().octic_linear_d8_wgrad_finish(o._p(ws), splits, cin, cout, o._arr5(w32) if scaled else None,
                                                 o._arr5(cs) if scaled else None, o._p(bias if scaled else None), o._p(dysum),
                                                 o._arr5(dw), o._arr5(dcs) if scaled else None, o._p(dbias), o._stream(ws)))
    torch.cuda.synchronize()
    for i in range(5):
        untouched(dwb[i][0], f"{what}: the row in front of dW {NAMES[i]}")
        untouched(dwb[i][-1], f"{what}: the row behind dW {NAMES[i]}")
        written(dw[i], f"{what}: dW {NAMES[i]}")
        exact(dw[i], (p.dw5[i] if scaled else p.g5[i]).float(), f"{what}: dW {NAMES[i]}")
        untouched(dcsb[i][0::2], f"{what}: the rows around dcs {NAMES[i]}")
        if scaled:
            exact(dcs[i], p.dcs5[i].float(), f"{what}: dcs {NAMES[i]}")
        else:
            untouched(dcs[i], f"{what}: dcs {NAMES[i]} of a finish without cs")
    untouched(dbb[0::2], f"{what}: the rows around dbias")
    exact(dbias, (p.dbias if scaled else p.dysum).float(), f"{what}: dbias")


WGRAD_CASES = [(cin, cout, "f32" if dt == f32 else "bf16") for (cin, cout), (_, dts) in WGRAD.items() for dt in dts]


@gpu
@pytest.mark.parametrize("cin,cout,dtype", WGRAD_CASES)
def test_weight_gradient(cin, cout, dtype):
    """wgrad_kernel<TIN, TT> / wgrad_ring_kernel + wgrad_finish_kernel with `splits` passed through the C ABI."""
    o, L = ops(), lib()
    dt = f32 if dtype == "f32" else bf
    tile = WGRAD[(cin, cout)][0]
    ring = dt == bf and cin % 160 == 0 and cout % 160 == 0
    for M, _ in ROWS:
        p = wgrad_problem(M, cin, cout)
        wgrad_plan_is(M, cin, cout, dt, WG_RING if ring else WG_TILED, tile)
        x, dy = with_tail(p.x5, dt, 3.0), with_tail(p.dy5, dt, 2.0)
        xv, dyv = o.pview(x, cin), o.pview(dy, cout)
        dysum = o.colsum_a1(dyv, M, cout, dt, dy)
        exact(dysum, p.dysum.float(), f"M {M}: octic_colsum_a1")
        for splits in SPLITS:
            what = f"M {M}, {cin} -> {cout}, splits {splits}"
            n = L.lib().octic_linear_d8_wgrad_workspace_bytes(cin, cout, splits) // 4
            ws = sentinel((n + WS_GUARD,), f32)
            L.check(L.lib().octic_linear_d8_wgrad(ctypes.byref(xv), ctypes.byref(dyv), M, cin, cout, code(dt), o._p(ws), splits,
                                                  o._stream(x)))
            torch.cuda.synchronize()
            untouched(ws[n:], f"{what}: behind the workspace")
            run_finish(o, p, ws, splits, False, dysum, what + ", finish without cs")
            run_finish(o, p, ws, splits, True, dysum, what + ", finish with cs and dysum")
            if ring:
                run_finish(o, p, ws, splits, True, None, what + ", finish with the kernel's own column sums")
                run_finish(o, p, ws, splits, False, None, what + ", finish without cs, the kernel's own column sums")
            untouched(ws[n:], f"{what}: behind the workspace after the finishes")
