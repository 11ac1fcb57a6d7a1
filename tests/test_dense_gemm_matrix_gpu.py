"""csrc/dense_gemm.hip: every epilogue (mode 0 .. 6) under every tile schedule, on operands whose products and partial sums
are EXACT in f32 in any summation order - a dropped or doubled K-tile, a swapped slab, a wrong row map or column set is then
a wrong number, not noise.

Operands (problem()): A integers in [-3, 3]; B integers in [-2, 2] times 2^-s with s = round(log2(sqrt(8 K))) - the sum of K
products has variance 8 K, so the pre-activations come out at unit scale and GELU / GELU' are not saturated (asserted: at
least 95 % inside (-3, 3)), and |acc| <= 6 K 2^-s is an integer below 2^24 times a power of two; bias in quarters; gamma a
power of two; rs in {0, 2}; X integers.  The reference is plain torch in float64 with the ONE rounding the kernel makes
(f32 -> bf16 of an exactly known value), so modes 0 / 1 (C) / 2 / 5 are compared bit for bit.  GELU and GELU' outputs are held
to |got - want| <= 1.2 * 2^-8 * max(1, |want|) against float64: half a bf16 ulp of the result plus the margin
test_dense_nt_gelu_factor_pair already allows dg_gelu / dg_gelu_both / dg_gelu_grad.

Split-K is forced through OCTIC_ROUTE_DENSE_SPLIT (set before the first launch of the shape, restored in finally;
_lib.route_override drops the cached workspaces), and every case asserts through ops.dense_plan that the launch is the
schedule it is named after - a knob that silently did nothing fails there."""
import contextlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GELU_BOUND = 1.2 * 2.0 ** -8
MODES = tuple(range(7))
RPS = 50                                    # token rows per sample of rs (mode 2)
SENTINEL = 0x5A5B                           # bf16 bit pattern of the guard cells


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


@contextlib.contextmanager
def routed(**knobs):
    """Routing knobs (split / tile / image / cls2) for the launches inside, back to automatic afterwards."""
    L = lib()
    ids = {"split": L.ROUTE_DENSE_SPLIT, "tile": L.ROUTE_DENSE_TILE, "image": L.ROUTE_DENSE_IMAGE, "cls2": L.ROUTE_DENSE_CLS2}
    try:
        for k, v in knobs.items():
            L.route_override(ids[k], v)
        yield
    finally:
        for k in knobs:
            L.route_override(ids[k], 0)


def split_knob_is(value):
    """The split knob holds `value` (route_override returns what it replaces) - where the grid alone cannot tell."""
    L = lib()
    assert L.route_override(L.ROUTE_DENSE_SPLIT, value) == value, "OCTIC_ROUTE_DENSE_SPLIT is not in force"


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def split_grid(M, N, K, s, tile=256):
    """Workgroups of a launch with fewer tiles than CUs whose every tile is cut s ways (at least 4 K-tiles per part)."""
    tiles = -(-M // 256) * -(-N // tile)
    assert tiles < cus()
    return (tiles * min(s, max(1, K // 64 // 4)) + 7) & ~7


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


class Problem:
    pass


_LAST = {}


def problem(M, N, K):
    """Exact operands and the float64 reference of one shape (kept for the cases of that shape that follow; never modified)."""
    if _LAST.get("key") == (M, N, K):
        return _LAST["p"]
    _LAST.clear()
    g = torch.Generator(device=DEV).manual_seed(1000003 * M + 1009 * N + K)
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g, device=DEV)
    p = Problem()
    p.M, p.N, p.K = M, N, K
    s = round(0.5 * math.log2(8.0 * K))       # = round(log2(sqrt(8 K))), with the ties (K = 256, 4096) computed exactly
    p.a = ri(-3, 3, M, K).to(torch.bfloat16)
    p.b = (ri(-2, 2, N, K).double() * 2.0 ** -s).to(torch.bfloat16)
    p.bias = ri(-4, 4, N).float() / 4
    p.gamma = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], device=DEV)[ri(0, 5, N)]
    ns = -(-M // RPS)
    p.rs = 2.0 * ri(0, 1, ns).float()
    p.rs[0], p.rs[1] = 0.0, 2.0
    p.x = ri(-8, 8, M, N).float()
    p.h3 = torch.randn(M, N, generator=g, device=DEV).to(torch.bfloat16)
    p.h5 = (torch.rand(M, N, generator=g, device=DEV) * 1.4 - 0.2).to(torch.bfloat16)
    assert p.b.double().mul(2.0 ** s).frac().abs().max() == 0 and 6 * K < 2 ** 24
    acc = p.a.double() @ p.b.double().t()
    pre = acc + p.bias.double()
    assert torch.equal(pre.float().double(), pre) and torch.equal(acc.float().double(), acc)      # exactly known f32 values
    share = float(((pre > -3) & (pre < 3)).double().mean())
    assert share >= 0.95, f"pre-activations are not at unit scale: {share:.3f} inside (-3, 3)"
    p.hb = pre.float().to(torch.bfloat16)
    p.accb = acc.float().to(torch.bfloat16)
    rsrow = p.rs.double().repeat_interleave(RPS)[:M, None]
    p.out2 = (p.x.double() + rsrow * p.gamma.double() * p.hb.double()).float()
    p.out2n = (p.x.double() + p.accb.double()).float()
    p.want5 = (p.h5.float() * p.accb.float()).to(torch.bfloat16)
    p.want3 = (dgelu64(p.h3.double()) * p.accb.double()).to(torch.bfloat16)
    _LAST["key"], _LAST["p"] = (M, N, K), p
    return p


def exact(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()
        rows, cols = idx[:, 0], idx[:, 1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements wrong, rows {int(rows.min())}..{int(rows.max())}, "
                             f"columns {int(cols.min())}..{int(cols.max())}; first {idx[0].tolist()} got {float(got[tuple(idx[0])])} "
                             f"want {float(want[tuple(idx[0])])}")


def within(got, want, what, scale=None):
    """|got - want| <= 1.2 * 2^-8 * max(1, |want|) (times `scale` elementwise), want in float64."""
    bound = GELU_BOUND * want.abs().clamp(min=1.0)
    if scale is not None:
        bound = bound * scale
    worst = float(((got.double() - want).abs() / bound).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"


def colsum_ok(cs, c, what):
    want = c.double().sum(0)
    err = float((cs.double() - want).abs().max())
    assert err <= 1e-5 * max(1.0, float(c.double().abs().sum(0).max())), f"{what}: column sums off by {err:.3e}"


def run_mode(o, p, mode, tokens=0, a=None, b=None):
    """One mode of one problem through ops.dense_gemm_nt with every variant the mode has; asserts the results and returns
    the tensors of the launches (for bitwise repeatability)."""
    a = p.a if a is None else a
    b = p.b if b is None else b
    kw = dict(tokens=tokens)
    if mode == 0:
        c = o.dense_gemm_nt(a, b, 0, bias=p.bias, **kw)
        c0 = o.dense_gemm_nt(a, b, 0, **kw)
        exact(c, p.hb, "mode 0")
        exact(c0, p.accb, "mode 0 without bias")
        return c, c0
    if mode == 1:
        c, y = o.dense_gemm_nt(a, b, 1, bias=p.bias, **kw)
        exact(c, p.hb, "mode 1 pre-activation")
        within(y, gelu64(p.hb.double()), "mode 1 gelu")
        return c, y
    if mode == 6:
        y = o.dense_gemm_nt(a, b, 6, bias=p.bias, **kw)
        exact(y, o.dense_gemm_nt(a, b, 1, bias=p.bias, **kw)[1], "mode 6 against the gelu output of mode 1")
        within(y, gelu64(p.hb.double()), "mode 6 gelu")
        return (y,)
    if mode == 4:
        f, y = o.dense_gemm_nt(a, b, 4, bias=p.bias, **kw)
        within(f, dgelu64(p.hb.double()), "mode 4 gelu'")
        within(y, gelu64(p.hb.double()), "mode 4 gelu")
        return f, y
    if mode == 2:
        c, out = o.dense_gemm_nt(a, b, 2, bias=p.bias, gamma=p.gamma, rs=p.rs, rps=RPS, x=p.x, **kw)
        cn, outn = o.dense_gemm_nt(a, b, 2, x=p.x, **kw)
        exact(c, p.hb, "mode 2 branch")
        exact(out, p.out2, "mode 2 stream")
        exact(cn, p.accb, "mode 2 branch without bias / gamma / rs")
        exact(outn, p.out2n, "mode 2 stream without bias / gamma / rs")
        return c, out, cn, outn
    h = p.h3 if mode == 3 else p.h5
    c = o.dense_gemm_nt(a, b, mode, h=h, **kw)
    cc, cs = o.dense_gemm_nt(a, b, mode, h=h, want_colsum=True, **kw)
    cs2 = o.dense_gemm_nt(a, b, mode, h=h, want_colsum=True, **kw)[1]
    if mode == 5:
        exact(c, p.want5, "mode 5")
    else:
        within(c, p.want3.double(), "mode 3", scale=p.accb.double().abs().clamp(min=1.0))
    exact(cc, c, f"mode {mode} with column sums")
    colsum_ok(cs, c, f"mode {mode}")
    assert torch.equal(cs, cs2), f"mode {mode}: column sums differ between two launches"
    return c, cs


def plan_is(o, p, mode, grid, tile=256, image=False, tokens=0):
    got = o.dense_plan(p.M, p.N, p.K, mode, tokens)
    assert (got[0], got[2], got[3]) == (tile, image, grid), f"plan {got} is not tile {tile}, per-image {image}, grid {grid}"
    return got


def other_shape_launch(o):
    """Another (M, N, K) between two launches under test, as test_dense_nt_320_wide_tile_is_bitwise_repeatable does."""
    q = torch.ones((130, 512), dtype=torch.bfloat16, device=DEV)
    o.dense_gemm_nt(q, q[:72], 0)


def pairs(shapes, modes=MODES):
    return [(*s, m) if isinstance(s, tuple) else (s, m) for s in shapes for m in modes]


# ---- 1. unsplit, K of 2 / 3 / 4 K-tiles: the ring never reaches its steady state ------------------------------------------
@pytest.mark.parametrize("K,mode", pairs((128, 192, 256)))
def test_unsplit_short_k(K, mode):
    """300 x 264: 2 x 2 tiles, a last panel of 44 rows, a last column tile of 8 columns."""
    o, p = ops(), problem(300, 264, K)
    plan_is(o, p, mode, grid=4)
    run_mode(o, p, mode)


# ---- 2. forced split-K ---------------------------------------------------------------------------------------------------
SPLITS = ((512, 2), (1280, 2), (1280, 3), (1280, 4), (1280, 5), (2048, 3), (2048, 8))


@pytest.mark.parametrize("K,s,mode", pairs(SPLITS))
def test_forced_split(K, s, mode):
    """Parts of 4 / 10 / 6+7+7 / 5 / 4 / 10+11+11 / 4 K-tiles (odd lengths, odd first K-tiles): every mode's epilogue in
    the last arriver, twice with another shape in between - the ticket is re-armed and the slab order is fixed."""
    o = ops()
    with routed(split=s):
        p = problem(300, 264, K)
        split_knob_is(s)
        plan_is(o, p, mode, grid=split_grid(300, 264, K, s))
        first = run_mode(o, p, mode)
        other_shape_launch(o)
        again = run_mode(o, p, mode)
    for x, y in zip(first, again):
        assert torch.equal(x, y), "two launches of a forced split differ"


def test_split_knob_at_zero_leaves_a_short_k_unsplit():
    """The same shape as the first forced case: without the knob there is one workgroup per tile."""
    o, p = ops(), problem(300, 264, 512)
    plan_is(o, p, 0, grid=4)
    run_mode(o, p, 0)


# ---- 3. forced split on the 320-wide tile --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (320, 640))
@pytest.mark.parametrize("s", (2, 5))
def test_forced_split_on_both_tile_widths(N, s):
    o = ops()
    res = {}
    for nt, width in ((5, 320), (4, 256)):
        with routed(split=s, tile=nt):
            p = problem(300, N, 1280)
            split_knob_is(s)
            plan_is(o, p, 0, grid=split_grid(300, N, 1280, s, width), tile=width)
            res[nt] = run_mode(o, p, 0)
            other_shape_launch(o)
            for x, y in zip(res[nt], run_mode(o, p, 0)):
                assert torch.equal(x, y)
    for x, y in zip(res[4], res[5]):
        assert torch.equal(x, y)


# ---- 4. the unsplit thin tail kept in front of the grid ------------------------------------------------------------------
@pytest.mark.parametrize("mode", (0, 2, 5))
def test_front_unsplit_thin_tail(mode):
    """32 full panels + one of 20 rows, 8 column tiles: 264 tiles on 256 CUs is one whole round and 8 tiles left, all of the
    20-row panel.  Knob = 1 keeps them unsplit in FRONT of the grid (8 workgroups, then the 256 full tiles)."""
    if cus() != 256:
        pytest.skip(f"the shape is one round + the thin panel only on 256 CUs (this device has {cus()})")
    M, N, K = 32 * 256 + 20, 2048, 128
    o = ops()
    tiles, n_cu = 33 * 8, cus()
    rem = tiles - tiles // n_cu * n_cu
    assert rem == 8
    with routed(split=1):
        p = problem(M, N, K)
        split_knob_is(1)              # (front or back, the grid is 264 workgroups: the plan cannot tell, the knob can)
        plan_is(o, p, mode, grid=((rem + 7) & ~7) + tiles - rem)
        run_mode(o, p, mode)


# ---- 5. the model's own split, fused tails, not a ViT-H shape ------------------------------------------------------------
@pytest.mark.parametrize("mode", (1, 2, 3, 5))
def test_natural_split_fused_tails(mode):
    """3000 x 520 x 4096 with no knob: 12 x 3 tiles cut seven ways on 256 CUs (the shape of the plain repeatability test)."""
    if cus() != 256:
        pytest.skip(f"the plan asserted here is the 256-CU one (this device has {cus()})")
    o, p = ops(), problem(3000, 520, 4096)
    plan_is(o, p, mode, grid=(36 * 7 + 7) & ~7)
    first = run_mode(o, p, mode)
    other_shape_launch(o)
    for x, y in zip(first, run_mode(o, p, mode)):
        assert torch.equal(x, y)


# ---- 6. per-image panels + the class-token kernels -----------------------------------------------------------------------
@pytest.mark.parametrize("B,N,K,mode", pairs(((3, 272, 256), (17, 320, 768))))
def test_per_image_panels(B, N, K, mode):
    """Exact results on the patch rows AND the class-token rows (exact operands: the class-token kernel's other summation
    order cannot matter), column sums over the plan's 2 B + ceil(B / 16) slab rows.  Mode 2 stays on classic panels."""
    o = ops()
    with routed(image=1):
        p = problem(B * 257, N, K)
        if mode == 2:
            plan_is(o, p, 2, grid=-(-p.M // 256) * -(-N // 256), tokens=257)
        else:
            width = o.dense_plan(p.M, N, K, mode, 257)[0]
            assert width == 256 or (mode == 0 and N % 320 == 0)
            got = plan_is(o, p, mode, grid=B * -(-N // width), tile=width, image=True, tokens=257)
            assert got[1] == 2 * B + (B + 15) // 16
        run_mode(o, p, mode, tokens=257)


@pytest.mark.parametrize("K,image", ((640, True), (960, False)))
def test_per_image_class_token_rows_as_two_launches(K, image):
    """OCTIC_ROUTE_DENSE_CLS2 = 2: the class-token rows as partial tiles over K slices of 320 + a summing launch.  Per-image
    panels need K % 128 == 0 and the two launches K % 320 == 0, so K = 640 is the smallest K that takes them; K = 960 (a
    multiple of 320 only) is refused by the plan and must stay on classic panels whatever the knobs say."""
    o = ops()
    with routed(image=1, cls2=2):
        p = problem(5 * 257, 640, K)
        width = o.dense_plan(p.M, 640, K, 0, 257)[0]
        tiles_m = 5 if image else -(-p.M // 256)
        plan_is(o, p, 0, grid=tiles_m * -(-640 // width), tile=width, image=image, tokens=257)
        run_mode(o, p, 0, tokens=257)


# ---- row edges: the 16-row MFMA tile, the 64-row half, the 128-row wave row ----------------------------------------------
@pytest.mark.parametrize("r,mode", pairs((1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255)))
def test_row_edges(r, mode):
    o, p = ops(), problem(256 + r, 264, 128)
    plan_is(o, p, mode, grid=4)
    run_mode(o, p, mode)


@pytest.mark.parametrize("r,mode", pairs((1, 17, 65, 129)))
def test_row_edges_under_a_forced_split(r, mode):
    o = ops()
    with routed(split=3):
        p = problem(256 + r, 264, 1280)
        split_knob_is(3)
        plan_is(o, p, mode, grid=split_grid(256 + r, 264, 1280, 3))
        run_mode(o, p, mode)


# ---- nothing outside [M, N] is written -----------------------------------------------------------------------------------
def _guarded_bf16(M, N, inner=None):
    t = torch.full((M + 8, N + 8), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    if inner is not None:
        t[:M, :N] = inner
    return t


def _guards_intact(t, M, N, what):
    bits = t.view(torch.int16)
    assert bool((bits[M:] == SENTINEL).all()), f"{what}: rows past M were written"
    assert bool((bits[:M, N:] == SENTINEL).all()), f"{what}: columns past N were written"


GUARD = [("unsplit", 300, 264, 256, m) for m in (0, 2, 3, 4)] + [("split3", 300, 264, 1280, m) for m in (0, 2, 3, 4)] + \
        [("image", 3 * 257, 272, 256, m) for m in (0, 3, 4)]


@pytest.mark.parametrize("schedule,M,N,K,mode", GUARD)
def test_nothing_outside_the_problem_is_written(schedule, M, N, K, mode):
    """Through the C ABI with outputs larger than the problem (ldc = N + 8), prefilled with a sentinel: the guard rows and
    columns keep it, the [M, N] block holds the exact result, every column-sum row the plan announces has been written."""
    o, L = ops(), lib()
    knobs = {"unsplit": {}, "split3": {"split": 3}, "image": {"image": 1}}[schedule]
    tokens = 257 if schedule == "image" else 0
    nan = float("nan")
    with routed(**knobs):
        p = problem(M, N, K)
        if schedule == "split3":
            split_knob_is(3)
        grid = {"unsplit": 4, "split3": split_grid(M, N, K, 3), "image": 3 * 2}[schedule]
        plan = plan_is(o, p, mode, grid=grid, image=schedule == "image", tokens=tokens)
        ws = o._dense_ws(M, N, K, p.a.device)
        c, c2 = _guarded_bf16(M, N), _guarded_bf16(M, N)
        h = _guarded_bf16(M, N, p.h3)
        out = torch.full((M + 8, N), nan, device=DEV)
        cs = torch.full((plan[1] + 4, N), nan, device=DEV)
        bias = p.bias if mode != 3 else None
        gamma, rs, x = (p.gamma, p.rs, p.x) if mode == 2 else (None, None, None)
        P = o._p
        L.check(L.lib().octic_dense_gemm_nt_tokens(P(p.a), P(p.b), M, N, K, K, K, mode, P(c), P(c2) if mode == 4 else None, N + 8,
                                                   P(bias), P(gamma), P(rs), RPS, P(x), P(out) if mode == 2 else None,
                                                   P(h) if mode == 3 else None, P(cs) if mode == 3 else None, P(ws), tokens,
                                                   o._stream(p.a)))
        torch.cuda.synchronize()
    for name, t in (("C", c), ("C2", c2), ("H", h)):
        _guards_intact(t, M, N, name)
    assert bool(out[M:].isnan().all()), "OUT: rows past M were written"
    got = c[:M, :N]
    if mode == 0:
        exact(got, p.hb, "C")
    elif mode == 2:
        exact(got, p.hb, "C")
        exact(out[:M], p.out2, "OUT")
    elif mode == 4:
        within(got, dgelu64(p.hb.double()), "C = gelu'")
        within(c2[:M, :N], gelu64(p.hb.double()), "C2 = gelu")
    else:
        within(got, p.want3.double(), "C", scale=p.accb.double().abs().clamp(min=1.0))
        exact(h[:M, :N], p.h3, "H")
        assert bool(cs[plan[1]:].isnan().all()), "column-sum rows past the plan's were written"
        assert not bool(cs[:plan[1]].isnan().any()), "a column-sum row the plan announces was not written"
        colsum_ok(cs[:plan[1]].double().sum(0), got, "column-sum slabs")
    if mode != 2:
        assert bool(out.isnan().all())
    if mode != 4:
        assert bool((c2.view(torch.int16) == SENTINEL).all())
    if mode != 3:
        assert bool(cs.isnan().all())


# ---- operands with a row stride ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,s", ((256, 0), (1280, 2)))
@pytest.mark.parametrize("mode", (0, 2))
def test_row_stride_operands(K, s, mode):
    """A = columns 8 .. 8 + K of an [M, K + 64] tensor, B likewise of [N, K + 32] (16-byte aligned pointers, lda > K, ldb > K),
    the surrounding columns filled with a large value: the same bits as contiguous copies.  Rows past M / N still read as
    zeros - the buffer descriptors end at M * lda / N * ldb."""
    o = ops()
    M, N = 300, 264
    with routed(**({"split": s} if s else {})):
        p = problem(M, N, K)
        if s:
            split_knob_is(s)
        plan_is(o, p, mode, grid=split_grid(M, N, K, s) if s else 4)
        aw = torch.full((M, K + 64), 3.0, dtype=torch.bfloat16, device=DEV)
        bw = torch.full((N, K + 32), 2.0, dtype=torch.bfloat16, device=DEV)
        aw[:, 8:8 + K] = p.a
        bw[:, 8:8 + K] = p.b
        a, b = aw[:, 8:8 + K], bw[:, 8:8 + K]
        assert a.stride(0) == K + 64 and b.stride(0) == K + 32 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0
        strided = run_mode(o, p, mode, a=a, b=b)
        dense = run_mode(o, p, mode)
    for x, y in zip(strided, dense):
        assert torch.equal(x, y)
