"""The dense weight-gradient family dW[N, K] = dY[M, N]^T X[M, K] (csrc/dense_wgrad.hip: dense_tn_kernel<4 | 5, false | true>,
dense_tn_narrow_kernel + dense_tn_narrow_finish) through the C ABI (octic_dense_wgrad_tn_skip, octic_dense_wgrad_tn_pair_skip and
the workspace queries) on operands whose products and partial sums are EXACT in f32 in any summation order.  Every comparison is
bit for bit against float64 (`!=`, so +0 equals -0): one dropped or doubled reduction step, a slab summed twice, a tile written
to the wrong place, a row behind M let in is a wrong number, not noise.  The only tolerance in this file is the derived summation
bound of test_random_operands.

Operands (seeded from the shape, generated on the CPU)
  dyadic (the default): dy = k / 4 with k an integer in [-8, 8], x = k / 4 with k in [-12, 12].  Exact in bf16; every product is a
    multiple of 1/16, every partial and total sum j / 16 with |j| <= 96 M.  exact_product asserts 96 M < 2^24 and, in float64,
    that the result survives an f32 round trip.  Reference: dy.double().t() @ x.double().  Holds whatever the slab count, tile
    width, step order or mask.
  selector (full-mantissa transport, M <= N): dy[m, sel(m)] = +-2^e, e in [-2, 2], 0 elsewhere, sel injective, seeded and not
    monotone; x = randn in bf16 with every mantissa bit live somewhere.  A dW row has at most one term: dW[sel(m), :] =
    +-2^e x[m, :] exactly, every other row exactly 0.  And the mirror image (x a selector on K, dy arbitrary).  What the LDS-DMA,
    the XOR swizzle and the transposing reads carry arrives with all its bits or the test fails.
  random (one small case per kernel, secondary): randn bf16 against the float64 product of the same bf16 values under the
    per-element bound 2 M 2^-23 (|dY|^T |X|)[n, k] (the summation bound of tests/test_octic_wgrad_skip_gpu.py: M additions and M
    products, each within one f32 ulp = 2^-23 relative of a partial sum that |dY|^T |X| bounds).  The largest observed fraction
    of the bound is printed.
  tails: every operand is the first M rows of a buffer with TAIL = 64 further rows of NaN (the wide kernel stages 64 rows a step,
    the narrow one 32); strided operands also have NaN in their padding columns.  A row or column guard that lets them in is a
    NaN in the result.

Guards.  dW is prefilled with NaN and has one guard row in front and one behind: afterwards every cell is written and every
guard cell still holds its NaN bits (compared as int32).  The workspace is the test's own: 4096 bytes of zeros (the tickets), a
NaN-filled slab region (an unpublished partial that gets summed shows) and WS_GUARD NaN floats behind
octic_dense_wgrad(_pair)_workspace_bytes.  After every launch and a synchronize the guard is untouched and THE TICKET REGION IS
ALL ZERO AGAIN (the last arriver of a tile re-arms its ticket; a miss would corrupt a later launch of another shape).  Every case
asserts (tile width, tiles, row slabs) through octic_dense_wgrad_plan before it launches; OCTIC_ROUTE_WGRAD_SLABS is set inside
try / finally and back at 0 afterwards.  tests/test_dense_wgrad_matrix_host.py checks the tables below against the plan queries
without a GPU.

Shapes (workload-sized M = 16448, slabs of more than 64 steps and the training-step comparisons stay with test_dense_gemm_gpu.py,
test_wgrad_skip_gpu.py and test_baselines_gpu.py)
  1. STEPS_M: steps per slab, one tile, S forced to 1, N = 256, K = 256 | 320: nkt = 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6 - the prologue
     of 4 and of 6 units, both ring halves, drain only (nkt <= 2) and the first steady iterations, ragged last steps.
  2. SLABS: (M, forced S, S the launcher must pick, steps of each slab): uneven steps * s / S boundaries; (130, 2) must clamp to
     1, (2049, 0) is the automatic 16.  Each case runs three times (the last arriver's own slab index varies): bitwise equal.
  3. DECODE_256 / DECODE_320: (N / 256, K / tile width) with 1 .. 17 tiles (every r8 = tiles & 7 with q8 = tiles >> 3 in 0, 1, 2)
     at DECODE_MS = (M, forced S) = (130, 1), (321, 2), (321, 3).
  4. PAIR: N0, N1 in PAIR_N x K in PAIR_K, plus PAIR_EXTRA = (1280, 256, 256): (N0 / 256) (K / width) over PAIR_N x PAIR_K is
     1, 2, 3, 4, 6, and the first tile of problem 1 is to sit at every tiles0 = 1 .. 6, so the 5 gets a case of its own.
     PAIR_MS = (65, 1), (321, 2).  Four operands with four different row strides (pair_layout), dw0 and dw1 guarded separately,
     each result also bitwise the single launch's (exactness).
  5. strides: column slices at element offset 8 and 264 of buffers with ld = N + 8 and ld = 3 N + 16 (16-byte aligned, neither 32-
     nor 256-byte), dy and x as slices of ONE fused buffer; dW a view inside a larger f32 buffer (the guard rows).
  6. MASKED: (rows_per_sample, sample counts, forced S): every one of the 2^B masks for B <= 5, the named masks of
     test_wgrad_skip_gpu._masks and three seeded ones otherwise.  dY rows of dropped samples are zero, X is NaN in every step
     that lies wholly inside dropped samples; the result equals float64 exactly and the unmasked launch bit for bit.  Slabs with
     0, 1, 2 and 3 live steps occur at both tile widths.  One pair case under every mask of 5 samples.
  7. NARROW_NK x NARROW_M: 64 x 64 tiles, slabs [M s / S, M (s + 1) / S) that fall inside a 32-row stage; S = 1 up to 129 rows,
     2 at 257, 8 at 1027, the cap 32 at 4099; ld = N + 8 operands; a mask changes nothing."""
import contextlib
import functools

import pytest
import torch

from test_wgrad_skip_gpu import _masks               # the named stochastic-depth masks (imports without a GPU)

gpu = pytest.mark.gpu

DEV = "cuda"
bf, f32 = torch.bfloat16, torch.float32
STEP = 64                                            # token rows per reduction step of the wide kernel (DW_BR)
STAGE = 32                                           # token rows per LDS stage of the narrow kernel (DWN_R)
TAIL = 64                                            # NaN rows behind every operand
WS_GUARD = 4096                                      # NaN floats behind the workspace
TICKETS = 1024                                       # int32 words of the ticket region (4096 bytes)
NAN_BITS = 0x7FC00000                                # what torch.full(.., nan) writes
MAX_SLABS = 16                                       # the launcher's cap, forced or automatic

WIDE_NK = ((256, 256), (256, 320))                   # one tile of either width

# ---- 1. steps per slab
STEPS_M = (1, 63, 64, 65, 127, 128, 129, 192, 193, 257, 321)
STEPS_NKT = (1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 6)

# ---- 2. (M, forced S, S of the plan, steps per slab)
SLABS = ((130, 2, 1, (3,)),
         (257, 2, 2, (2, 3)),
         (449, 3, 3, (2, 3, 3)),
         (641, 5, 5, (2, 2, 2, 2, 3)),
         (1153, 9, 9, (2,) * 8 + (3,)),
         (2049, 16, 16, (2,) * 15 + (3,)),
         (2049, 0, 16, (2,) * 15 + (3,)))
REPEATS = 3

# ---- 3. (N / 256, K / tile width); (M, forced S)
DECODE_256 = ((1, 1), (2, 1), (1, 3), (2, 2), (5, 1), (3, 2), (7, 1), (4, 2), (3, 3), (5, 2), (11, 1), (4, 3), (13, 1), (7, 2),
              (5, 3), (4, 4), (17, 1))
DECODE_320 = ((1, 1), (3, 1), (1, 3), (5, 1), (7, 1), (3, 3))
DECODE_MS = ((130, 1), (321, 2), (321, 3))

# ---- 4. pair
PAIR_N = (256, 512, 768)
PAIR_K = (256, 512, 320)
PAIR_EXTRA = ((1280, 256, 256),)                     # (N0, N1, K): tiles0 = 5
PAIR_MS = ((65, 1), (321, 2))
PAIR_MASKED = (64, 5, 512, 256, 256, 2)              # rows_per_sample, B, N0, N1, K, forced S

# ---- 5. strides
STRIDED_M = 193
STRIDED_S = (1, 2)
NARROW_STRIDED = ((61, 128, 64), (257, 64, 192), (1027, 192, 192))      # (M, N, K) with ld = N + 8 | K + 8

# ---- 6. (rows_per_sample, sample counts, forced S)
MASKED = {"64-row samples": (64, (1, 2, 3, 4, 5), (1, 2)),
          "65-row samples": (65, (5,), (1, 2)),
          "1-row samples": (1, (129,), (1,)),
          "37-row samples": (37, (7,), (1, 2))}
EVERY_MASK_UP_TO = 5

# ---- 7. narrow
NARROW_NK = ((64, 64), (128, 64), (64, 192), (192, 192), (320, 192))
NARROW_M = (1, 31, 32, 33, 127, 129, 257, 1027, 4099)
NARROW_MASK = (257, 128, 64, 1)                      # M, N, K, rows_per_sample of the masked call
NARROW_CUS = 256                                     # compute units the slab rule of the narrow path counts (MI355X)

# ---- selector and random operands: (M, N, K)
SELECTOR = ((193, 256, 256), (193, 256, 320), (61, 64, 128))
RANDOM = ((321, 256, 256), (321, 256, 320), (257, 128, 64))


def ops():
    from octic_vits_amd import ops as o
    return o


def lib():
    from octic_vits_amd import _lib
    return _lib


# ---- what the launcher is to pick, restated ---------------------------------------------------------------------------------
def steps_of(M):
    return -(-M // STEP)


def width_of(N, K):
    """Tile width of the plan: 256 wherever it divides K, 320 for K % 320 == 0 only, 64 on the narrow path."""
    if N % 256 == 0 and K % 256 == 0:
        return 256
    if N % 256 == 0 and K % 320 == 0:
        return 320
    return 64


def tiles_of(N, K):
    w = width_of(N, K)
    return (N // (64 if w == 64 else 256)) * (K // w)


def forced_slabs(M, forced):
    """Row slabs of a wide launch under OCTIC_ROUTE_WGRAD_SLABS = forced > 0: at most 16, at least two steps per slab."""
    return max(1, min(forced, MAX_SLABS, steps_of(M) // 2))


def slab_steps(M, S):
    """(first step, end step) of every slab: [steps s / S, steps (s + 1) / S)."""
    steps = steps_of(M)
    return [(steps * s // S, steps * (s + 1) // S) for s in range(S)]


def narrow_slabs(M, tiles):
    """dwn_slabs: about two workgroups per CU, at most 32, at least four 32-row stages per slab."""
    return max(1, min(-(-2 * NARROW_CUS // tiles), 32, -(-M // STAGE) // 4))


def step_is_live(M, rps, mask, j):
    """The kernel's liveness rule: step j is walked if one of its token rows belongs to a sample whose factor is non-zero."""
    r0, r1 = j * STEP, min(j * STEP + STEP, M)
    return any(mask[r0 // rps:(r1 - 1) // rps + 1])


def live_steps(M, rps, mask, S):
    """Live steps of every slab."""
    return [sum(step_is_live(M, rps, mask, j) for j in range(s0, s1)) for s0, s1 in slab_steps(M, S)]


def every_mask(B):
    return {format(m, f"0{B}b"): [2.0 * ((m >> b) & 1) for b in range(B)] for m in range(2 ** B)}


def masks_of(B):
    return every_mask(B) if B <= EVERY_MASK_UP_TO else _masks(B)


def decode(tiles, j):
    """Item j of a slab -> tile, the kernel's tile-list decode (None: a padding item)."""
    x, l, q8, r8 = j & 7, j >> 3, tiles >> 3, tiles & 7
    if l >= q8 + (1 if x < r8 else 0):
        return None
    return (x * (q8 + 1) if x < r8 else r8 * (q8 + 1) + (x - r8) * q8) + l


# ---- operands (CPU, float64 holding bf16 values) ---------------------------------------------------------------------------
def _generator(tag, *dims):
    seed = tag
    for d in dims:
        seed = seed * 1000003 + d
    return torch.Generator().manual_seed(seed % (2 ** 62))


def assert_exact_range(M):
    assert 96 * M < 2 ** 24, f"M = {M}: 16 times a sum of M products within [-6, 6] is no longer an f32 integer"


def is_bf16(t):
    return torch.equal(t.to(bf).double(), t)


def exact_product(dy, x):
    """dy^T x in float64, checked to be an f32 value (so every f32 summation order gives it)."""
    assert_exact_range(dy.shape[0])
    assert is_bf16(dy) and is_bf16(x)
    want = dy.t() @ x
    assert torch.equal(want.float().double(), want), "the operand ranges are too wide for this M"
    return want


@functools.lru_cache(maxsize=48)
def dyadic(M, N, K, tag=0):
    g = _generator(1 + tag, M, N, K)
    dy = torch.randint(-8, 9, (M, N), generator=g).double() / 4
    x = torch.randint(-12, 13, (M, K), generator=g).double() / 4
    return dy, x, exact_product(dy, x)


def selector(M, C, g):
    """[M, C] with one +-2^e per row in a column of its own (seeded, not monotone)."""
    assert M <= C
    sel = torch.randperm(C, generator=g)[:M]
    assert sel.unique().numel() == M and (M < 3 or bool((sel[1:] < sel[:-1]).any() and (sel[1:] > sel[:-1]).any()))
    e = torch.randint(-2, 3, (M,), generator=g).double()
    sign = torch.randint(0, 2, (M,), generator=g).double() * 2 - 1
    s = torch.zeros(M, C, dtype=torch.float64)
    s[torch.arange(M), sel] = sign * 2.0 ** e
    return s


def full_mantissa(M, C, g):
    """randn in bf16 (as float64) with every mantissa bit set somewhere and clear somewhere."""
    t = torch.randn(M, C, generator=g).to(bf)
    bits = t.view(torch.int16)
    for b in range(7):                                   # the 7 explicit mantissa bits of bf16
        one = (bits >> b) & 1
        assert bool(one.any()) and not bool(one.all())
    return t.double()


@functools.lru_cache(maxsize=8)
def selector_problem(M, N, K, mirror):
    g = _generator(7 + int(mirror), M, N, K)
    if mirror:
        dy, x = full_mantissa(M, N, g), selector(M, K, g)
    else:
        dy, x = selector(M, N, g), full_mantissa(M, K, g)
    want = dy.t() @ x                                    # at most one term per element
    assert is_bf16(dy) and is_bf16(x) and torch.equal(want.float().double(), want)
    assert int((want != 0).sum()) > 0
    return dy, x, want


# ---- device placement --------------------------------------------------------------------------------------------------------
def nan(shape, dtype=f32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def device_rows(vals, ld=None, off=0):
    """vals [M, C] as columns [off, off + C) of the first M rows of a bf16 buffer [M + TAIL, ld] that is NaN everywhere else."""
    M, C = vals.shape
    ld = C if ld is None else ld
    assert off + C <= ld and ld % 8 == 0 and off % 8 == 0
    buf = torch.full((M + TAIL, ld), float("nan"), dtype=bf)
    buf[:M, off:off + C] = vals.to(bf)
    return buf.to(DEV)[:M, off:off + C]


def fused_rows(dy, x):
    """dy and x as slices at element offsets 8 and 264 of ONE buffer with ld = 3 N + 16, as the fused QKV gradient hands them over."""
    M, N = dy.shape
    K = x.shape[1]
    ld = 3 * N + 16
    assert 8 + N <= 264 and 264 + K <= ld
    buf = torch.full((M + TAIL, ld), float("nan"), dtype=bf)
    buf[:M, 8:8 + N] = dy.to(bf)
    buf[:M, 264:264 + K] = x.to(bf)
    d = buf.to(DEV)
    return d[:M, 8:8 + N], d[:M, 264:264 + K]


def pair_strides(N0, N1, K):
    """(ld, offset) of dy0, x0, dy1, x1: four different row strides, both offsets, both stride rules."""
    want = [(N0 + 8, 8), (3 * K + 16, 264), (3 * N1 + 16, 8), (K + 8, 8)]
    out, used = [], set()
    for ld, off in want:
        while ld in used:
            ld += 8
        used.add(ld)
        out.append((ld, off))
    return out


def pair_layout(dy0, x0, dy1, x1):
    lds = pair_strides(dy0.shape[1], dy1.shape[1], x0.shape[1])
    views = [device_rows(t, ld, off) for t, (ld, off) in zip((dy0, x0, dy1, x1), lds)]
    assert len({v.stride(0) for v in views}) == 4
    return views


# ---- guards and comparisons --------------------------------------------------------------------------------------------------
def untouched(t, what):
    bad = t.view(torch.int32) != NAN_BITS
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} guard cells were written"


def written(t, what):
    bad = t.isnan()
    if bool(bad.any()):
        idx = bad.nonzero()
        raise AssertionError(f"{what}: {int(bad.sum())} of {t.numel()} cells are NaN (not written, or a NaN operand row or column got "
                             f"in), rows {int(idx[:, 0].min())}..{int(idx[:, 0].max())}, columns {int(idx[:, 1].min())}.."
                             f"{int(idx[:, 1].max())}")


def exact(got, want, what):
    assert got.dtype == want.dtype == f32 and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()
        rows, cols = idx[:, 0], idx[:, 1]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements wrong, rows {int(rows.min())}..{int(rows.max())}, "
                             f"columns {int(cols.min())}..{int(cols.max())}; first {idx[0].tolist()} got {float(got[tuple(idx[0])])} "
                             f"want {float(want[tuple(idx[0])])}")


def on_device(want64):
    return want64.float().to(DEV)


def workspace(nbytes):
    """[zeroed tickets | NaN slabs | NaN guard] as f32; n = floats up to the guard."""
    assert nbytes % 4 == 0 and nbytes >= 4 * TICKETS
    n = nbytes // 4
    ws = nan((n + WS_GUARD,))
    ws[:TICKETS] = 0
    return ws, n


def workspace_is_clean(ws, n, what):
    untouched(ws[n:], f"{what}: behind the workspace")
    left = ws[:TICKETS].view(torch.int32)
    assert not bool(left.any()), f"{what}: {int((left != 0).sum())} tickets are not back at zero, first at tile {int(left.nonzero()[0])}"


def guarded_dw(N, K):
    buf = nan((N + 2, K))
    return buf, buf[1:N + 1]


def dw_is_whole(buf, what):
    untouched(buf[0], f"{what}: the row in front of dW")
    untouched(buf[-1], f"{what}: the row behind dW")
    written(buf[1:-1], what)


@contextlib.contextmanager
def slabs_knob(value):
    """OCTIC_ROUTE_WGRAD_SLABS for the launches inside; back at 0 afterwards, and checked to be."""
    L = lib()
    try:
        L.route_override(L.ROUTE_WGRAD_SLABS, value)
        yield
    finally:
        L.route_override(L.ROUTE_WGRAD_SLABS, 0)
    assert L.route_override(L.ROUTE_WGRAD_SLABS, 0) == 0


def plan_is(M, N0, N1, K, ld_max, width, tiles, S):
    got = lib().plan("octic_dense_wgrad_plan", M, N0, N1, K, ld_max)
    assert got == (width, tiles, S, 0), f"M {M}, N {N0} + {N1}, K {K}: the plan is {got}, this case is about {(width, tiles, S, 0)}"


def mask_args(mask, rps):
    if mask is None:
        return None, 0
    return torch.tensor(mask, dtype=f32, device=DEV), rps


# ---- launches ----------------------------------------------------------------------------------------------------------------
def run_single(dyv, xv, want, S, what, mask=None, rps=0):
    """One octic_dense_wgrad_tn_skip launch into a guarded dW from a guarded workspace; returns dW [N, K]."""
    o, L = ops(), lib()
    (M, N), K = dyv.shape, xv.shape[1]
    plan_is(M, N, 0, K, max(dyv.stride(0), xv.stride(0)), width_of(N, K), tiles_of(N, K), S)
    ws, n = workspace(int(L.lib().octic_dense_wgrad_workspace_bytes(M, N, K)))
    buf, dw = guarded_dw(N, K)
    ss, rps = mask_args(mask, rps)
    L.check(L.lib().octic_dense_wgrad_tn_skip(o._p(dyv), o._p(xv), M, N, K, dyv.stride(0), xv.stride(0), o._p(dw), o._p(ss), rps,
                                              o._p(ws), o._stream(dw)))
    torch.cuda.synchronize()
    workspace_is_clean(ws, n, what)
    dw_is_whole(buf, what)
    if want is not None:
        exact(dw, want, what)
    return dw


def run_pair(views, want0, want1, S, what, mask=None, rps=0):
    """One octic_dense_wgrad_tn_pair_skip launch; dw0 and dw1 guarded separately; returns (dW0, dW1)."""
    o, L = ops(), lib()
    dy0, x0, dy1, x1 = views
    (M, N0), N1, K = dy0.shape, dy1.shape[1], x0.shape[1]
    width = width_of(N0 + N1, K)
    plan_is(M, N0, N1, K, max(v.stride(0) for v in views), width, ((N0 + N1) // 256) * (K // width), S)
    ws, n = workspace(int(L.lib().octic_dense_wgrad_pair_workspace_bytes(M, N0, N1, K)))
    (buf0, dw0), (buf1, dw1) = guarded_dw(N0, K), guarded_dw(N1, K)
    ss, rps = mask_args(mask, rps)
    L.check(L.lib().octic_dense_wgrad_tn_pair_skip(o._p(dy0), o._p(x0), N0, dy0.stride(0), x0.stride(0), o._p(dw0), o._p(dy1),
                                                   o._p(x1), N1, dy1.stride(0), x1.stride(0), o._p(dw1), M, K, o._p(ss), rps,
                                                   o._p(ws), o._stream(dw0)))
    torch.cuda.synchronize()
    workspace_is_clean(ws, n, what)
    dw_is_whole(buf0, what + ", dW0")
    dw_is_whole(buf1, what + ", dW1")
    exact(dw0, want0, what + ", dW0")
    exact(dw1, want1, what + ", dW1")
    return dw0, dw1


def run_dyadic(M, N, K, forced, S, what=None, tag=0):
    dy, x, want = dyadic(M, N, K, tag)
    with slabs_knob(forced):
        return run_single(device_rows(dy), device_rows(x), on_device(want), S, what or f"M {M}, {N} x {K}, S {S}")


# ---- 1. steps per slab -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", WIDE_NK)
def test_steps_per_slab(N, K):
    """One tile, one slab of 1 .. 6 steps: every prologue length, drain-only and steady loops, full and ragged last steps."""
    for M in STEPS_M:
        run_dyadic(M, N, K, 1, 1)


# ---- 2. row slabs ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", WIDE_NK)
@pytest.mark.parametrize("M,forced,S", [row[:3] for row in SLABS])
def test_row_slabs(M, forced, S, N, K):
    """Uneven slab boundaries, the ticket and the last arriver's sum in slab order: exact, and the same bits every time."""
    first = run_dyadic(M, N, K, forced, S)
    for i in range(1, REPEATS):
        exact(run_dyadic(M, N, K, forced, S), first, f"M {M}, {N} x {K}, S {S}: run {i} against run 0")


# ---- 3. tile-list decode -----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,forced", DECODE_MS)
@pytest.mark.parametrize("width", (256, 320))
def test_tile_list_decode(width, M, forced):
    """1 .. 17 tiles: every remainder of the 8-way deal of the tile list, padding items, tiles of both problems' columns."""
    for a, b in (DECODE_256 if width == 256 else DECODE_320):
        N, K = 256 * a, width * b
        assert width_of(N, K) == width and tiles_of(N, K) == a * b
        run_dyadic(M, N, K, forced, forced_slabs(M, forced), f"M {M}, {N} x {K} ({a * b} tiles), S {forced}")


# ---- 4. pair launch ----------------------------------------------------------------------------------------------------------
PAIR_CASES = [(N0, N1, K) for K in PAIR_K for N0 in PAIR_N for N1 in PAIR_N] + list(PAIR_EXTRA)


def pair_problem(M, N0, N1, K):
    dy0, x0, want0 = dyadic(M, N0, K, 0)
    dy1, x1, want1 = dyadic(M, N1, K, 1)                          # (a second activation, not x0 again)
    return (dy0, x0, dy1, x1), on_device(want0), on_device(want1)


@gpu
@pytest.mark.parametrize("K", PAIR_K)
def test_pair_launch(K):
    """The joint tile list [problem 0 | problem 1] with the seam at tiles0 = 1 .. 6, from four strided operands; each result is
    also the single launch's, bit for bit."""
    for N0, N1, k in PAIR_CASES:
        if k != K:
            continue
        for M, forced in PAIR_MS:
            S = forced_slabs(M, forced)
            cpu, want0, want1 = pair_problem(M, N0, N1, K)
            views = pair_layout(*cpu)
            what = f"pair M {M}, {N0} + {N1} x {K}, S {S}"
            with slabs_knob(forced):
                dw0, dw1 = run_pair(views, want0, want1, S, what)
                exact(dw0, run_single(views[0], views[1], want0, S, what + ", problem 0 alone"), what + ": dW0 against the single launch")
                exact(dw1, run_single(views[2], views[3], want1, S, what + ", problem 1 alone"), what + ": dW1 against the single launch")


# ---- 5. strides --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", WIDE_NK)
def test_strided_operands_wide(N, K):
    """Column slices at offsets 8 and 264, ld = N + 8 and 3 N + 16, NaN in every padding column and behind row M."""
    M = STRIDED_M
    dy, x, want = dyadic(M, N, K)
    want = on_device(want)
    layouts = {"ld + 8": (device_rows(dy, N + 8, 8), device_rows(x, K + 8, 8)), "fused": fused_rows(dy, x)}
    assert layouts["fused"][0].stride(0) == layouts["fused"][1].stride(0) == 3 * N + 16
    for name, (dyv, xv) in layouts.items():
        assert dyv.data_ptr() % 32 == 16 and xv.data_ptr() % 32 == 16
        for forced in STRIDED_S:
            with slabs_knob(forced):
                run_single(dyv, xv, want, forced_slabs(M, forced), f"{name}: M {M}, {N} x {K}, S {forced}")


@gpu
def test_strided_operands_narrow():
    for M, N, K in NARROW_STRIDED:
        dy, x, want = dyadic(M, N, K)
        run_single(device_rows(dy, N + 8, 8), device_rows(x, K + 8, 8), on_device(want), narrow_slabs(M, tiles_of(N, K)),
                   f"narrow ld + 8: M {M}, {N} x {K}")


# ---- 6. masked instantiation -------------------------------------------------------------------------------------------------
def masked_problem(dy, x, mask, rps):
    """(dY with the rows of dropped samples zeroed, X with NaN in every step wholly inside dropped samples, float64 result)."""
    M = dy.shape[0]
    keep = (torch.tensor(mask) != 0).repeat_interleave(rps)
    dyz = dy * keep[:, None].double()
    xp = x.clone()
    for j in range(steps_of(M)):
        if not step_is_live(M, rps, mask, j):
            xp[j * STEP:j * STEP + STEP] = float("nan")
    return dyz, xp, exact_product(dyz, x)


@gpu
@pytest.mark.parametrize("N,K", WIDE_NK)
@pytest.mark.parametrize("table", list(MASKED))
def test_masked_launch(table, N, K):
    """dense_tn_kernel<KW, true>: the live steps of every slab, and only those, in the unmasked launch's grouping."""
    rps, counts, slabs = MASKED[table]
    for B in counts:
        M = B * rps
        dy, x, _ = dyadic(M, N, K)
        for name, mask in masks_of(B).items():
            dyz, xp, want = masked_problem(dy, x, mask, rps)
            want = on_device(want)
            dyv, xv, xpv = device_rows(dyz), device_rows(x), device_rows(xp)
            for forced in slabs:
                S = forced_slabs(M, forced)
                what = f"{table}, B {B}, mask {name}, {N} x {K}, S {S}"
                with slabs_knob(forced):
                    plain = run_single(dyv, xv, want, S, what + ", unmasked")
                    got = run_single(dyv, xpv, want, S, what + ", masked", mask, rps)
                exact(got, plain, what + ": masked against unmasked")


@gpu
def test_masked_pair_launch():
    rps, B, N0, N1, K, forced = PAIR_MASKED
    M = B * rps
    S = forced_slabs(M, forced)
    (dy0, x0, dy1, x1), _, _ = pair_problem(M, N0, N1, K)
    for name, mask in every_mask(B).items():
        z0, p0, want0 = masked_problem(dy0, x0, mask, rps)
        z1, p1, want1 = masked_problem(dy1, x1, mask, rps)
        want0, want1 = on_device(want0), on_device(want1)
        what = f"pair under mask {name}"
        with slabs_knob(forced):
            w0, w1 = run_pair(pair_layout(z0, x0, z1, x1), want0, want1, S, what + ", unmasked")
            g0, g1 = run_pair(pair_layout(z0, p0, z1, p1), want0, want1, S, what + ", masked", mask, rps)
        exact(g0, w0, what + ": dW0 masked against unmasked")
        exact(g1, w1, what + ": dW1 masked against unmasked")


# ---- 7. narrow kernel --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N,K", NARROW_NK)
def test_narrow_kernel(N, K):
    """64 x 64 tiles: slabs that begin and end inside a 32-row stage (the r < r1 guard), 1 .. 32 of them, and the finish kernel."""
    tiles = tiles_of(N, K)
    assert width_of(N, K) == 64
    for M in NARROW_M:
        S = narrow_slabs(M, tiles)
        dy, x, want = dyadic(M, N, K)
        run_single(device_rows(dy), device_rows(x), on_device(want), S, f"narrow M {M}, {N} x {K}, S {S}")


@gpu
def test_a_mask_changes_nothing_on_the_narrow_path():
    M, N, K, rps = NARROW_MASK
    dy, x, want = dyadic(M, N, K)
    want = on_device(want)
    S = narrow_slabs(M, tiles_of(N, K))
    dyv, xv = device_rows(dy), device_rows(x)
    plain = run_single(dyv, xv, want, S, "narrow, unmasked")
    for name, mask in _masks(M // rps, seeds=(1,)).items():
        exact(run_single(dyv, xv, want, S, f"narrow, mask {name}", mask, rps), plain, f"narrow, mask {name}")


# ---- selector and random operands --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mirror", (False, True), ids=("dy selects", "x selects"))
@pytest.mark.parametrize("M,N,K", SELECTOR)
def test_full_mantissa_transport(M, N, K, mirror):
    """One term per output element: the other operand's bf16 values arrive scaled by a power of two with every bit, or not at all."""
    dy, x, want = selector_problem(M, N, K, mirror)
    want = on_device(want)
    wide = width_of(N, K) != 64
    for forced in ((1, 2) if wide else (0,)):
        S = forced_slabs(M, forced) if wide else narrow_slabs(M, tiles_of(N, K))
        with slabs_knob(forced):
            run_single(device_rows(dy), device_rows(x), want, S, f"selector M {M}, {N} x {K}, S {S}")


@gpu
@pytest.mark.parametrize("M,N,K", RANDOM)
def test_random_operands(M, N, K):
    """randn operands under the derived bound 2 M 2^-23 (|dY|^T |X|); the observed fraction of it is printed, not tuned."""
    g = _generator(11, M, N, K)
    dy, x = torch.randn(M, N, generator=g).to(bf).double(), torch.randn(M, K, generator=g).to(bf).double()
    want, bound = dy.t() @ x, 2.0 * M * 2.0 ** -23 * (dy.abs().t() @ x.abs())
    wide = width_of(N, K) != 64
    S = lib().plan("octic_dense_wgrad_plan", M, N, 0, K, max(N, K))[2]
    assert S == (min(MAX_SLABS, steps_of(M) // 2) if wide else narrow_slabs(M, tiles_of(N, K)))
    got = run_single(device_rows(dy), device_rows(x), None, S, f"random M {M}, {N} x {K}").double().cpu()
    err = (got - want).abs()
    print(f"\nrandom operands, M {M}, {N} x {K} (tile {width_of(N, K)}, S {S}): largest error / bound = {float((err / bound).max()):.4f}")
    assert bool((bound > 0).all())
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} elements beyond the summation bound, worst {float((err / bound).max()):.3f} of it"
