"""Every row kernel of csrc/dense.hip through the C ABI, at every chunk count (NV = ceil(d / 256) = 1..8), lane edge, row
edge, grid cap and row map, against float64 torch on the CPU.

Kernels: LayerNorm forward / backward (predicated and wide), the fused residual-add + LayerNorm, the fused
LayerNorm-backward + residual tail, the layer-scale / stochastic-depth tail forward and backward, their row-map variants,
the GELU backward with its bias sums, the bf16 column sums and the slab reduction (octic_dense_finish[_batch]).

Shape tables (tests/test_dense_rows_host.py checks that they reach every template instance of every routing branch)
  WHOLE   256, 512, ... 2048           NV 1..8, every lane live in every chunk
  EDGE    256 (NV-1) + 4, 256 NV - 4   one lane, and all lanes but one, in the last chunk: 4, 252, 260, 508, ... 1796, 2044
  EXTRA   384                          ViT-S
  width sweep     every width above at 67 rows (5 slabs of 16 waves, the last with 3 rows; 5 forward workgroups)
  row sweep       rows 1, 3, 5, 16, 17, 67, 257, 4115 (= 256 x 16 + 19: past the 256-slab cap) at one EDGE and one WHOLE width
                  per kernel path (ROW_SWEEP_WIDTHS)
  grid caps       65553 rows at d = 4 and d = 256: past the 4096 workgroups of the forward and the 8192 of the fused forward
  samples         rows_per_scale = rps_of(rows) in the sweeps (1 at 67 rows, 5 at 4115), and SAMPLE_CASES: 3 (rows a multiple
                  of 3; 3 divides no workgroup's 16 rows) and rows itself (one sample)
  relations       RELATION_WIDTHS (WHOLE <= 1280 and the EDGE widths 4, 508, 1796) x rows 67 and 4115
  colsum          d = 8, 504, 512, 520, 3840 inside ld = d + 8; rows -> strip ceil(rows / 256) of a slab:
                  3 -> 1, 700 -> 3 (fewer than 4 rows), 4096 -> 16, 4100 -> 17, 7419 -> 29 (= 16 + 13)
  gelu_bwd        d = 8, 504, 512, 520, 5120 x rows 1, 3, 1030, 2309 (= 256 x 9 + 5: strip 10, two-row trip then tail loop)
  finish          nblocks 1, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 255, 256 x d 4, 8, 12, 260

Operands and references.  Every reference is float64 on the CPU from the inputs the kernel reads (rounded to bf16 first
where the kernel reads bf16).
  exact (compared with !=, no tolerance)
    tail forward / backward   x integers in [-8, 8], y in [-3, 3], gout in [-4, 4], gamma from {+-0.5, +-1, +-2}, rs from
                              {0, 2} (samples 0 and 1 are 0 and 2; a single sample is 2): out = x + rs gamma y,
                              gy = rs gamma gout (a multiple of 0.5, |gy| <= 16: exact in bf16), dgamma = sum rs gout y,
                              colsum = gamma sum rs gout are exact in f32 in any summation order (|sum| <= 24 rows < 2^24)
    db of every LayerNorm backward   gy is integers in [-3, 3] in every LayerNorm-backward case of this file
    colsum, finish            integers; the finished sums are bit exact, and the batch equals the single launches
    all-zero row              y = b (bf16(b)) bit for bit, mean = 0, rstd = rsqrtf(eps) within 2 f32 ulp of float64 eps^-0.5
  toleranced (the bounds of tests/test_dense_gpu.py; model-scale inputs x = 0.5 + 3 N(0,1), w = 1 + 0.3 N, b = 0.2 N,
  dres = N)
    f32 y            rtol = atol = 2e-5                      mean    rtol = atol = 1e-5
    rstd             relative 2e-5 against float64 1/sqrt(var + eps): a function of the same row sums as y, so the bound
                     of the f32 output
    bf16 y, gyb, dh  |got - ref| <= t + 2^-8 |ref|: one rounding (half a bf16 ulp) of an f32 value within t of ref; t is the
                     f32 bound of the same quantity (y, dh: 2e-5 (1 + |ref|); gyb = rs gamma dx: |rs gamma| 1e-4 + 1e-4 |ref|)
    xout             rtol = atol = 2e-6
    dx               rtol = atol = 1e-4
    dw, and dgamma / colsum of the tail kernel   rtol 1e-4, atol 1e-4 sqrt(rows), against float64 of the whole formula
    gelu column sums against the float64 sum of the kernel's own stored dh: rtol 1e-6, atol 2^-22 x sum |dh| of the column
  bit for bit between kernels (torch.equal)
    fused forward = scale_residual_fwd then layernorm_fwd (stream, y, stats), four (yb, y) dtype pairs, with and without
    gamma / rs; fused backward tail = layernorm_bwd then scale_residual_bwd (dx, gyb; the four sums to 1e-5 of their scale:
    other slab order); every row-map kernel = the plain kernel on gathered rows, scattered back (sums included: the
    row-to-wave assignment depends on the row count only).  Maps: a non-monotonic permutation of a strict subset with gaps
    that holds the stream's first and last row, the identity, one row; the stream holds 2 to 3 times the map's rows.

Measured on an MI355X (largest over all cases; no fallback bound of any quantity was needed): rstd 3.0e-6 relative, 0.025
of its 2e-5 bound; f32 y 2.3e-6, mean 6.0e-7, xout 1.0e-6 (0.12 of its bound), dx 6.5e-7, dw / dgamma / colsum 1.3e-2 of
theirs; dh of gelu_bwd within 0.99 of t + 2^-8 |ref| with the f32 bound t = 2e-5 (1 + |ref|); the gelu column sums 0.078 of
2^-22 x sum |dh| + 1e-6 |ref|.  Every bit-for-bit relation holds at every width and row count of the tables.

Guards.  Every output the test allocates (y, stats, xout, xcopy, dx, gy / gyb, dh, partial slabs, finished sums) has one
guard row in front and one behind and is prefilled with NaN (f32) or the bf16 pattern 0x5A5B; after the launch every cell
of the output is written and every guard cell holds the sentinel (for colsum / gelu_bwd the row behind the 256 slabs).  For
the row-map kernels the stream rows the map does not name play that role.  Every input has 16 rows of non-zero values
behind row `rows`.
"""
import ctypes
import functools
import itertools
import math
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-6
F32, BF16 = torch.float32, torch.bfloat16
DTYPES = (F32, BF16)
DTN = {F32: "f32", BF16: "bf16"}
SENT16 = 0x5A5B                                   # bf16 sentinel; f32 outputs are prefilled with NaN
TAIL_ROWS = 16                                    # non-zero rows behind every input

# ----------------------------------------------------------------------------------------------------------- tables
WHOLE = tuple(256 * nv for nv in range(1, 9))
EDGE = tuple(d for nv in range(1, 9) for d in (256 * (nv - 1) + 4, 256 * nv - 4))
EXTRA = (384,)
WIDTHS = tuple(sorted(WHOLE + EDGE + EXTRA))
SWEEP_ROWS = 67
ROW_SWEEP = (1, 3, 5, 16, 17, 67, 257, 4115)
CAP_ROWS, CAP_WIDTHS = 65553, (4, 256)
RELATION_WIDTHS = (256, 512, 768, 1024, 1280, 4, 508, 1796)
RELATION_ROWS = (67, 4115)
TAIL_WIDTHS = (256, 512, 768, 1024, 1280)         # what octic_dense_layernorm_bwd_tail accepts
# one EDGE and one WHOLE width per kernel path
ROW_SWEEP_WIDTHS = {
    "ln_fwd": (508, 512),                         # one (predicated) kernel
    "ln_bwd": (508, 512, 1792),                   # predicated with a partial chunk | wide | predicated, every lane live
    "resid_ln_fwd": (508, 512),                   # predicated | fast path
    "scale_residual": (508, 512),                 # predicated | fast path of the backward
    "ln_bwd_tail": (512,),                        # whole chunks only
}
SAMPLE_CASES = ((66, 3), (4113, 3), (67, 67), (4115, 4115))           # (rows, rows_per_scale)
GAMMAS = (0.5, -0.5, 1.0, -1.0, 2.0, -2.0)
COLSUM_WIDTHS = (8, 504, 512, 520, 3840)
COLSUM_ROWS = ((3, 1), (700, 7), (4096, 16), (4100, 4), (7419, 3))    # (rows, rows_per_sample of the _skip launch)
GELU_WIDTHS = (8, 504, 512, 520, 5120)
GELU_ROWS = (1, 3, 1030, 2309)
FINISH_NBLOCKS = (1, 15, 16, 17, 48, 49, 63, 64, 65, 112, 113, 255, 256)
FINISH_WIDTHS = (4, 8, 12, 260)
FINISH_MODES = ("out0", "out1", "both_scaled", "out1_scaled")


def rps_of(rows):
    """rows_per_scale of the sweeps: a small divisor of rows that does not divide a workgroup's 16 rows, else 1."""
    return next(k for k in (3, 5, 7, 1) if rows % k == 0)


def _sweep(path):
    return [(SWEEP_ROWS, d) for d in WIDTHS] + [(r, d) for d in ROW_SWEEP_WIDTHS[path] for r in ROW_SWEEP if r != SWEEP_ROWS]


LN_CASES = sorted(set(_sweep("ln_fwd") + _sweep("ln_bwd")))
RESID_LN_CASES = sorted(set(_sweep("resid_ln_fwd") + [(r, d) for d in RELATION_WIDTHS for r in RELATION_ROWS]))
SCALE_RESIDUAL_CASES = ([(r, rps_of(r), d) for r, d in _sweep("scale_residual")]
                        + [(r, k, d) for d in ROW_SWEEP_WIDTHS["scale_residual"] for r, k in SAMPLE_CASES])
TAIL_CASES = sorted(set([(SWEEP_ROWS, d) for d in TAIL_WIDTHS] + [(4115, d) for d in TAIL_WIDTHS]
                        + [(r, d) for d in ROW_SWEEP_WIDTHS["ln_bwd_tail"] for r in ROW_SWEEP]))
ROWMAP_CASES = ([(r, d, kind) for d in RELATION_WIDTHS for r in RELATION_ROWS for kind in ("subset", "identity")]
                + [(1, d, "one") for d in RELATION_WIDTHS])


def _id(v):
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------- ABI
def O():
    from octic_vits_amd import ops
    return ops


def LIB():
    from octic_vits_amd import _lib
    return _lib.lib()


def ck(code):
    O().check(code)


def p(t):
    return O()._p(t)


def code(dtype):
    return O().dt_code(dtype)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Out:
    """A [rows, width] output with one guard row in front and one behind, prefilled with the sentinel."""

    def __init__(self, rows, width, dtype=F32):
        if dtype == F32:
            self.buf = torch.full((rows + 2, width), float("nan"), dtype=F32, device=DEV)
        else:
            self.buf = torch.full((rows + 2, width), SENT16, dtype=torch.int16, device=DEV).view(BF16)
        self.sent = int(_bits(self.buf)[0, 0])
        self.body = self.buf[1:rows + 1]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.body.data_ptr())

    def check(self, name):
        b = _bits(self.buf)
        assert bool((b[0] == self.sent).all()) and bool((b[-1] == self.sent).all()), f"{name}: a guard row was written"
        if self.buf.dtype == F32:
            assert bool(torch.isfinite(self.body).all()), f"{name}: cells left unwritten (or not finite)"
        else:
            assert not bool((b[1:-1] == self.sent).any()), f"{name}: cells left unwritten"
        return self.body


def close(got, ref, rtol, atol, name, bf16=False, scale=None):
    """|got - ref| <= atol + rtol |ref| (+ 2^-8 |ref| for one bf16 rounding); atol may be a tensor; prints the worst ratio."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound = atol + rtol * ref.abs() + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max err {float(err.max()) if err.numel() else 0.0:.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{name}: err / bound up to {ratio:.3f}"


def exact(got, ref, name):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = got != ref                                      # (+0 equals -0; a NaN differs from everything)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} values differ, first at {bad.nonzero()[0].tolist()}"


def finish(part, nblk, d, want0=True, want1=True, scale1=None, name="finish"):
    """octic_dense_finish of nblk slabs [2][d] into guarded sums."""
    o0 = Out(1, d) if want0 else None
    o1 = Out(1, d) if want1 else None
    ck(LIB().octic_dense_finish(part if isinstance(part, ctypes.c_void_p) else p(part), nblk, d, o0.ptr if o0 else None,
                                o1.ptr if o1 else None, p(scale1), stream()))
    return (o0.check(name + " out0")[0] if o0 else None), (o1.check(name + " out1")[0] if o1 else None)


# ---------------------------------------------------------------------------------------------------------- inputs
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nonzero_tail(t, rows):
    t[rows:] = torch.where(t[rows:] == 0, torch.ones_like(t[rows:]), t[rows:])
    return t


def ints(g, lo, hi, rows, d):
    """Integers in [lo, hi] as f32, rows + TAIL_ROWS rows, the tail without zeros."""
    return _nonzero_tail(torch.randint(lo, hi + 1, (rows + TAIL_ROWS, d), generator=g).float(), rows)


def normal(g, rows, d, mul=1.0, add=0.0):
    return torch.randn(rows + TAIL_ROWS, d, generator=g) * mul + add


def pick(g, values, n):
    return torch.tensor(values)[torch.randint(0, len(values), (n,), generator=g)]


def exact_rs(g, samples):
    """rs from {0, 2}: samples 0 and 1 are 0 and 2, a single sample is 2; two non-zero entries behind the last sample."""
    rs = pick(g, (0.0, 2.0), samples + 2)
    rs[samples:] = 2.0
    if samples == 1:
        rs[0] = 2.0
    else:
        rs[0], rs[1] = 0.0, 2.0
    return rs


def row_scale(rs, rows, rps):
    """[rows, 1] float64 factor of every row (ones without rs)."""
    if rs is None:
        return torch.ones(rows, 1, dtype=torch.float64)
    return rs.double()[torch.arange(rows) // rps].view(rows, 1)


def ln_ref(x, w, b):
    """float64 LayerNorm of the rows of x: y, mean, rstd, xhat."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(1, keepdim=True) + EPS)
    xh = xc * rstd
    return xh * w.double() + b.double(), mean[:, 0], rstd[:, 0], xh


def ln_bwd_ref(gy, xh, rstd, w, dres):
    gy = gy.double()
    g = gy * w.double()
    dx = (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True)) * rstd.view(-1, 1)
    if dres is not None:
        dx = dx + dres.double()
    return dx, (gy * xh).sum(0), gy.sum(0)


@functools.lru_cache(maxsize=2)
def ln_case(rows, d):
    """Model-scale LayerNorm operands (CPU and device) and the float64 forward of the first `rows` rows."""
    g = _gen(1000 * d + rows)
    c = types.SimpleNamespace(rows=rows, d=d)
    c.x = normal(g, rows, d, 3.0, 0.5)
    c.w = torch.randn(d, generator=g) * 0.3 + 1
    c.b = torch.randn(d, generator=g) * 0.2
    c.gy = ints(g, -3, 3, rows, d)
    c.dres = normal(g, rows, d)
    c.y, c.mean, c.rstd, c.xh = ln_ref(c.x[:rows], c.w, c.b)
    c.dev = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("x", "w", "b", "gy", "dres")})
    return c


def ln_fwd(x, w, b, rows, d, dt, rowmap=None, want_copy=False, name="ln_fwd"):
    """octic_dense_layernorm_fwd[_rows] into guarded y / stats / xcopy."""
    y, st = Out(rows, d, dt), Out(rows, 2)
    xc = Out(rows, d) if want_copy else None
    if rowmap is None and not want_copy:
        ck(LIB().octic_dense_layernorm_fwd(p(x), y.ptr, code(dt), p(w), p(b), st.ptr, rows, d, EPS, stream()))
    else:
        ck(LIB().octic_dense_layernorm_fwd_rows(p(x), y.ptr, code(dt), p(w), p(b), st.ptr, rows, d, EPS, p(rowmap),
                                                xc.ptr if xc else None, stream()))
    y.check(name + " y")
    st.check(name + " stats")
    if xc:
        xc.check(name + " xcopy")
    return y.body, st.body, (xc.body if xc else None)


def check_ln_fwd(y, st, ref_y, ref_mean, ref_rstd, dt, name):
    close(y, ref_y, 2e-5, 2e-5, name + " y", bf16=dt == BF16)
    close(st[:, 0], ref_mean, 1e-5, 1e-5, name + " mean")
    close(st[:, 1], ref_rstd, 2e-5, 0.0, name + " rstd")


# ------------------------------------------------------------------------------------------- LayerNorm fwd / bwd
@pytest.mark.parametrize("dt", DTYPES, ids=DTN.get)
@pytest.mark.parametrize("rows,d", LN_CASES, ids=_id)
def test_layernorm_fwd_bwd(rows, d, dt):
    """Forward (y, mean, rstd) and backward (dx, dw, exact db) against float64; with and without dres / partials."""
    c = ln_case(rows, d)
    v = c.dev
    y, st, _ = ln_fwd(v.x, v.w, v.b, rows, d, dt)
    check_ln_fwd(y, st, c.y, c.mean, c.rstd, dt, "ln_fwd")
    nblk = LIB().octic_dense_blocks(rows)
    gy = v.gy.to(dt)
    dx, part = Out(rows, d), Out(nblk, 2 * d)
    ck(LIB().octic_dense_layernorm_bwd(p(gy), code(dt), p(v.x), p(v.w), p(st), p(v.dres), dx.ptr, part.ptr, rows, d, stream()))
    dx.check("ln_bwd dx")
    part.check("ln_bwd partials")
    dw, db = finish(part.ptr, nblk, d)
    ref_dx, ref_dw, ref_db = ln_bwd_ref(c.gy[:rows], c.xh, c.rstd, c.w, c.dres[:rows])
    close(dx.body, ref_dx, 1e-4, 1e-4, "ln_bwd dx")
    close(dw, ref_dw, 1e-4, 1e-4 * math.sqrt(rows), "ln_bwd dw")
    exact(db, ref_db, "ln_bwd db")
    dx2 = Out(rows, d)                                     # no residual cotangent, no parameter gradients
    ck(LIB().octic_dense_layernorm_bwd(p(gy), code(dt), p(v.x), p(v.w), p(st), None, dx2.ptr, None, rows, d, stream()))
    close(dx2.check("ln_bwd dx (no dres)"), ref_dx - c.dres[:rows].double(), 1e-4, 1e-4, "ln_bwd dx (no dres)")


@pytest.mark.parametrize("dt", DTYPES, ids=DTN.get)
@pytest.mark.parametrize("d", CAP_WIDTHS)
def test_layernorm_fwd_past_the_grid_cap(d, dt):
    """65553 rows: 4097 workgroups' worth against the cap of 4096, every wave a further trip."""
    rows = CAP_ROWS
    c = ln_case(rows, d)
    y, st, _ = ln_fwd(c.dev.x, c.dev.w, c.dev.b, rows, d, dt)
    check_ln_fwd(y, st, c.y, c.mean, c.rstd, dt, "ln_fwd")


# ------------------------------------------------------------------------------------- fused residual + LayerNorm
@functools.lru_cache(maxsize=2)
def resid_case(rows, d):
    g = _gen(2000 * d + rows)
    c = types.SimpleNamespace(rows=rows, d=d, rps=rps_of(rows))
    c.x = normal(g, rows, d, 3.0, 0.5)
    c.yb = normal(g, rows, d)
    c.gamma = torch.randn(d, generator=g) * 0.5
    samples = rows // c.rps
    c.rs = torch.bernoulli(torch.full((samples + 2,), 0.75), generator=g) / 0.75
    if samples > 1:
        c.rs[0], c.rs[1] = 0.0, 1 / 0.75
    c.w = torch.randn(d, generator=g) * 0.3 + 1
    c.b = torch.randn(d, generator=g) * 0.2
    c.dev = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("x", "yb", "gamma", "rs", "w", "b")})
    return c


def resid_ln_fwd(v, yb, gamma, rs, rps, rows, d, ydt, name="resid_ln_fwd"):
    xo, y, st = Out(rows, d), Out(rows, d, ydt), Out(rows, 2)
    ck(LIB().octic_dense_resid_layernorm_fwd(p(v.x), p(yb), code(yb.dtype), p(gamma), p(rs), rps, xo.ptr, y.ptr, code(ydt),
                                             p(v.w), p(v.b), st.ptr, rows, d, EPS, stream()))
    return xo.check(name + " xout"), y.check(name + " y"), st.check(name + " stats")


def check_resid_ln(c, rows, d, ybdt, ydt, with_gamma, with_rs, relation):
    v = c.dev
    yb = v.yb.to(ybdt)
    gamma, rs = (v.gamma if with_gamma else None), (v.rs if with_rs else None)
    name = f"resid_ln_fwd<{DTN[ybdt]},{DTN[ydt]}> gamma={with_gamma} rs={with_rs}"
    xo, y, st = resid_ln_fwd(v, yb, gamma, rs, c.rps, rows, d, ydt, name)
    if rows <= 257 or (with_gamma and with_rs and ybdt == ydt) or not relation:      # (float64 of 4115 rows: the full form only)
        s = row_scale(c.rs if with_rs else None, rows, c.rps) * (c.gamma.double() if with_gamma else 1.0)
        ref_x = c.x[:rows].double() + s * c.yb[:rows].to(ybdt).double()
        close(xo, ref_x, 2e-6, 2e-6, name + " xout")
        check_ln_fwd(y, st, *ln_ref(ref_x, c.w, c.b)[:3], ydt, name)
    if relation:
        out = O().scale_residual_fwd(v.x[:rows], yb[:rows], gamma, rs, c.rps)
        y2, st2 = O().dense_layernorm_fwd(out, v.w, v.b, EPS, ydt)
        assert torch.equal(xo, out), name + ": stream differs from scale_residual_fwd"
        assert torch.equal(y, y2), name + ": y differs from the two passes"
        assert torch.equal(st, st2), name + ": stats differ from the two passes"


@pytest.mark.parametrize("rows,d", RESID_LN_CASES, ids=_id)
def test_resid_layernorm_fwd(rows, d):
    """Stream, y and stats against float64 in all four (yb, y) dtype pairs with and without gamma / rs (at 4115 rows: the
    full form in the two equal-dtype pairs); at the relation shapes every combination also bit for bit against
    scale_residual_fwd followed by layernorm_fwd."""
    c = resid_case(rows, d)
    relation = d in RELATION_WIDTHS and rows in RELATION_ROWS
    for ybdt, ydt in itertools.product(DTYPES, DTYPES):
        for with_gamma, with_rs in ((True, True), (False, False), (True, False), (False, True)):
            check_resid_ln(c, rows, d, ybdt, ydt, with_gamma, with_rs, relation)


@pytest.mark.parametrize("d", CAP_WIDTHS)
def test_resid_layernorm_fwd_past_the_grid_cap(d):
    """65553 rows: 8195 workgroups' worth against the cap of 8192, every wave a further trip."""
    c = resid_case(CAP_ROWS, d)
    check_resid_ln(c, CAP_ROWS, d, BF16, F32, True, True, False)
    check_resid_ln(c, CAP_ROWS, d, F32, BF16, True, True, False)


# ---------------------------------------------------------------------------------------------- all-zero rows
@pytest.mark.parametrize("d", WIDTHS)
def test_all_zero_rows(d):
    """A row of zeros: y = b (bf16(b)) bit for bit, mean = 0, rstd = rsqrtf(eps) within 2 f32 ulp of float64 eps^-0.5."""
    rows, zr = SWEEP_ROWS, [0, 33, 66]
    c = resid_case(rows, d)
    v = c.dev
    x, yb = v.x.clone(), v.yb.clone()
    x[zr] = 0
    yb[zr] = 0
    ref = EPS ** -0.5
    ulp = float(torch.nextafter(torch.tensor(ref, dtype=F32), torch.tensor(float("inf"))) - torch.tensor(ref, dtype=F32))
    vz = types.SimpleNamespace(x=x, w=v.w, b=v.b)
    for dt in DTYPES:
        want = c.b.to(dt).double().expand(len(zr), d)
        runs = [("ln_fwd", ln_fwd(x, v.w, v.b, rows, d, dt)[:2])]
        for ybdt in DTYPES:
            runs.append((f"resid_ln_fwd<{DTN[ybdt]}>", resid_ln_fwd(vz, yb.to(ybdt), v.gamma, v.rs, c.rps, rows, d, dt)[1:]))
        for name, (y, st) in runs:
            name = f"{name} -> {DTN[dt]}"
            exact(y[zr], want, name + " y of a zero row")
            exact(st[zr, 0], torch.zeros(len(zr)), name + " mean of a zero row")
            err = (st[zr, 1].cpu().double() - ref).abs().max().item()
            assert err <= 2 * ulp, f"{name}: rstd of a zero row {err / ulp:.2f} ulp from eps^-0.5"


# ------------------------------------------------------------------------------------- layer-scale tail, exact
@functools.lru_cache(maxsize=2)
def tail_case(rows, rps, d):
    """Integer operands of the residual tail whose every result is exact in f32 (and in bf16 where it is stored so)."""
    assert 24 * rows < 2 ** 24
    g = _gen(3000 * d + 7 * rows + rps)
    c = types.SimpleNamespace(rows=rows, rps=rps, d=d)
    c.x = ints(g, -8, 8, rows, d)
    c.y = ints(g, -3, 3, rows, d)
    c.gout = ints(g, -4, 4, rows, d)
    c.gamma = pick(g, GAMMAS, d)
    c.rs = exact_rs(g, (rows + rps - 1) // rps)
    c.dev = types.SimpleNamespace(**{k: getattr(c, k).to(DEV) for k in ("x", "y", "gout", "gamma", "rs")})
    return c


def tail_refs(c, with_gamma, with_rs, gout=None):
    rows = c.rows
    s = row_scale(c.rs if with_rs else None, rows, c.rps)
    gm = c.gamma.double() if with_gamma else torch.ones(c.d, dtype=torch.float64)
    gout = c.gout[:rows].double() if gout is None else gout.double()
    y = c.y[:rows].double()
    return types.SimpleNamespace(out=c.x[:rows].double() + s * gm * y, gy=s * gm * gout, dgamma=(s * gout * y).sum(0),
                                 colsum=gm * (s * gout).sum(0))


def scale_residual_bwd(gout, y, gamma, rs, rps, rows, d, rowmap=None, want_partials=True, name="scale_residual_bwd"):
    nblk = LIB().octic_dense_blocks(rows)
    gy = Out(rows, d, y.dtype)
    part = Out(nblk, 2 * d) if want_partials else None
    ck(LIB().octic_scale_residual_bwd_rows(p(gout), p(y), code(y.dtype), p(gamma), p(rs), rps, gy.ptr,
                                           part.ptr if part else None, rows, d, p(rowmap), stream()))
    gy.check(name + " gy")
    if part:
        part.check(name + " partials")
    return gy.body, part, nblk


@pytest.mark.parametrize("ydt", DTYPES, ids=DTN.get)
@pytest.mark.parametrize("rows,rps,d", SCALE_RESIDUAL_CASES, ids=_id)
def test_scale_residual_exact(rows, rps, d, ydt):
    """out, gy, dgamma and colsum bit exact on integer operands, with and without gamma and rs; dgamma and colsum finished
    separately; gy again with partials = NULL (at whole-chunk widths <= 1280 the way out of the backward's fast path)."""
    c = tail_case(rows, rps, d)
    v = c.dev
    y = v.y.to(ydt)
    for with_gamma, with_rs in itertools.product((True, False), (True, False)):
        gamma, rs = (v.gamma if with_gamma else None), (v.rs if with_rs else None)
        ref = tail_refs(c, with_gamma, with_rs)
        name = f"<{DTN[ydt]}> gamma={with_gamma} rs={with_rs}"
        out = Out(rows, d)
        ck(LIB().octic_scale_residual_fwd(p(v.x), p(y), code(ydt), p(gamma), p(rs), rps, out.ptr, rows, d, stream()))
        exact(out.check("scale_residual_fwd" + name), ref.out, "scale_residual_fwd" + name)
        gy, part, nblk = scale_residual_bwd(v.gout, y, gamma, rs, rps, rows, d, name="scale_residual_bwd" + name)
        exact(gy, ref.gy, "scale_residual_bwd gy" + name)
        dgamma, none = finish(part.ptr, nblk, d, True, False, gamma)              # want_gamma alone
        exact(dgamma, ref.dgamma, "scale_residual_bwd dgamma" + name)
        none, colsum = finish(part.ptr, nblk, d, False, True, gamma)              # want_colsum alone
        exact(colsum, ref.colsum, "scale_residual_bwd colsum" + name)
        gy2, _, _ = scale_residual_bwd(v.gout, y, gamma, rs, rps, rows, d, want_partials=False)
        exact(gy2, ref.gy, "scale_residual_bwd gy without partials" + name)


# ------------------------------------------------------------------------- fused LayerNorm backward + residual tail
@pytest.mark.parametrize("rows,d", TAIL_CASES, ids=_id)
def test_layernorm_bwd_tail(rows, d):
    """octic_dense_layernorm_bwd_tail against float64 of the whole formula (dx, bf16 gyb, dw, exact db, dgamma, colsum) and
    against layernorm_bwd followed by scale_residual_bwd (dx, gyb bit for bit; the sums to 1e-5 of their scale)."""
    c, t = ln_case(rows, d), tail_case(rows, rps_of(rows), d)
    v, tv = c.dev, t.dev
    o = O()
    gy, yb = v.gy.bfloat16(), tv.y.bfloat16()
    _, st, _ = ln_fwd(v.x, v.w, v.b, rows, d, BF16)
    nblk = LIB().octic_dense_blocks(rows)
    for with_dres, with_gamma, with_rs in ((True, True, True), (False, False, False), (True, True, False), (False, False, True)):
        dres = v.dres if with_dres else None
        gamma, rs = (tv.gamma if with_gamma else None), (tv.rs if with_rs else None)
        name = f"ln_bwd_tail dres={with_dres} gamma={with_gamma} rs={with_rs}"
        dx, gyb, p1, p2 = Out(rows, d), Out(rows, d, BF16), Out(nblk, 2 * d), Out(nblk, 2 * d)
        ck(LIB().octic_dense_layernorm_bwd_tail(p(gy), p(v.x), p(v.w), p(st), p(dres), dx.ptr, p1.ptr, p(yb), p(gamma), p(rs),
                                                t.rps, gyb.ptr, p2.ptr, rows, d, stream()))
        for out, what in ((dx, "dx"), (gyb, "gyb"), (p1, "partials"), (p2, "partials2")):
            out.check(f"{name} {what}")
        dw, db = finish(p1.ptr, nblk, d)
        dgamma, colsum = finish(p2.ptr, nblk, d, scale1=gamma)
        ref_dx, ref_dw, ref_db = ln_bwd_ref(c.gy[:rows], c.xh, c.rstd, c.w, c.dres[:rows] if with_dres else None)
        ref = tail_refs(t, with_gamma, with_rs, gout=ref_dx)
        sg = row_scale(t.rs if with_rs else None, rows, t.rps) * (t.gamma.double() if with_gamma else 1.0)
        sq = math.sqrt(rows)
        close(dx.body, ref_dx, 1e-4, 1e-4, name + " dx")
        close(gyb.body, ref.gy, 1e-4, 1e-4 * sg.abs().expand(rows, d), name + " gyb", bf16=True)
        close(dw, ref_dw, 1e-4, 1e-4 * sq, name + " dw")
        exact(db, ref_db, name + " db")
        close(dgamma, ref.dgamma, 1e-4, 1e-4 * sq, name + " dgamma")
        close(colsum, ref.colsum, 1e-4, 1e-4 * sq, name + " colsum")
        dx2, dw2, db2 = o.dense_layernorm_bwd(gy[:rows], v.x[:rows], v.w, st, dres[:rows] if with_dres else None)
        gyb2, dgamma2, colsum2 = o.scale_residual_bwd(dx2, yb[:rows], gamma, rs, t.rps)
        assert torch.equal(dx.body, dx2), name + ": dx differs from layernorm_bwd"
        assert torch.equal(gyb.body, gyb2), name + ": gyb differs from scale_residual_bwd of that dx"
        for a, b, what in ((dw, dw2, "dw"), (db, db2, "db"), (dgamma, dgamma2, "dgamma"), (colsum, colsum2, "colsum")):
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), f"{name}: {what} against the two passes"


# ------------------------------------------------------------------------------------------------------ row maps
def make_map(rows, kind, seed):
    """(stream rows S, int64 map): the stream holds 2 to 3 times the map's rows."""
    g = _gen(seed)
    if kind == "identity":
        return 2 * rows, torch.arange(rows)
    if kind == "one":
        return 3, torch.tensor([1])
    S = 2 * rows + rows // 2 + 1
    inner = torch.randperm(S - 2, generator=g)[:rows - 2] + 1          # a strict subset with gaps ...
    m = torch.cat([inner, torch.tensor([0, S - 1])])                   # ... that holds the first and the last row
    m = m[torch.randperm(rows, generator=g)]
    assert len(set(m.tolist())) == rows and rows < S and bool((m[1:] < m[:-1]).any()) and bool((m[1:] > m[:-1]).any())
    return S, m


@pytest.mark.parametrize("rows,d,kind", ROWMAP_CASES, ids=_id)
def test_rowmap_layernorm(rows, d, kind):
    """layernorm_fwd_rows = layernorm_fwd of the gathered rows (y, stats, xcopy); layernorm_bwd_rows in place on the
    stream's cotangent = layernorm_bwd of the gathered rows scattered back, dw / db bit for bit, db exact, every row the
    map does not name untouched."""
    o = O()
    S, m = make_map(rows, kind, 17 * d + rows)
    g = _gen(4000 * d + rows)
    x = (torch.randn(S, d, generator=g) * 3 + 0.5).to(DEV)
    w, b = (torch.randn(d, generator=g) * 0.3 + 1).to(DEV), (torch.randn(d, generator=g) * 0.2).to(DEV)
    gy32 = ints(g, -3, 3, rows, d)
    g0 = torch.randn(S, d, generator=g).to(DEV)
    idx, rowmap = m.to(DEV), m.to(DEV).to(torch.int32)
    rest = torch.ones(S, dtype=torch.bool, device=DEV)
    rest[idx] = False
    nblk = LIB().octic_dense_blocks(rows)
    for dt in DTYPES:
        name = f"rows<{DTN[dt]}>"
        y, st, xa = ln_fwd(x, w, b, rows, d, dt, rowmap=rowmap, want_copy=True, name="ln_fwd_" + name)
        gathered = x[idx].contiguous()
        y2, st2 = o.dense_layernorm_fwd(gathered, w, b, EPS, dt)
        assert torch.equal(xa, gathered), name + ": xcopy is not the gathered rows"
        assert torch.equal(y, y2) and torch.equal(st, st2), name + ": forward differs from the gathered rows'"
        gy = gy32.to(DEV).to(dt)
        gs = g0.clone()
        part = Out(nblk, 2 * d)
        ck(LIB().octic_dense_layernorm_bwd_rows(p(gy), code(dt), p(xa), p(w), p(st), p(gs), p(gs), part.ptr, rows, d, p(rowmap),
                                                stream()))
        part.check(name + " partials")
        dw, db = finish(part.ptr, nblk, d)
        dx2, dw2, db2 = o.dense_layernorm_bwd(gy[:rows], gathered, w, st2, g0[idx].contiguous())
        assert torch.equal(gs[idx], dx2), name + ": in-place backward differs from the gathered rows'"
        assert torch.equal(_bits(gs[rest]), _bits(g0[rest])), name + ": a stream row outside the map changed"
        assert torch.equal(dw, dw2) and torch.equal(db, db2), name + ": dw / db differ from the gathered rows'"
        exact(db, gy32[:rows].double().sum(0), name + " db")


@pytest.mark.parametrize("rows,d,kind", ROWMAP_CASES, ids=_id)
def test_rowmap_scale_residual(rows, d, kind):
    """scale_residual_fwd_rows into the stream and scale_residual_bwd_rows from the stream's cotangent = the plain kernels on
    gathered rows (bit for bit, sums included) = the exact integer results; stream rows outside the map untouched."""
    o = O()
    S, m = make_map(rows, kind, 19 * d + rows)
    c = tail_case(rows, rps_of(rows), d)
    v = c.dev
    g = _gen(5000 * d + rows)
    s0 = torch.randint(-9, 10, (S, d), generator=g).float().to(DEV)
    idx, rowmap = m.to(DEV), m.to(DEV).to(torch.int32)
    rest = torch.ones(S, dtype=torch.bool, device=DEV)
    rest[idx] = False
    gstream = torch.randint(1, 5, (S, d), generator=g).float()                     # non-zero off the map
    gstream[m] = c.gout[:rows]
    gstream = gstream.to(DEV)
    ref = tail_refs(c, True, True)
    for ydt in DTYPES:
        name = f"rows<{DTN[ydt]}>"
        y = v.y.to(ydt)
        st = s0.clone()
        ck(LIB().octic_scale_residual_fwd_rows(p(v.x), p(y), code(ydt), p(v.gamma), p(v.rs), c.rps, p(st), rows, d, p(rowmap),
                                               stream()))
        out2 = o.scale_residual_fwd(v.x[:rows], y[:rows], v.gamma, v.rs, c.rps)
        assert torch.equal(st[idx], out2), name + ": forward differs from the plain kernel"
        assert torch.equal(_bits(st[rest]), _bits(s0[rest])), name + ": a stream row outside the map changed"
        exact(st[idx], ref.out, "scale_residual_fwd_" + name)
        gy, part, nblk = scale_residual_bwd(gstream, y, v.gamma, v.rs, c.rps, rows, d, rowmap=rowmap,
                                            name="scale_residual_bwd_" + name)
        dgamma, colsum = finish(part.ptr, nblk, d, scale1=v.gamma)
        gy2, dgamma2, colsum2 = o.scale_residual_bwd(v.gout[:rows], y[:rows], v.gamma, v.rs, c.rps)
        assert torch.equal(gy, gy2), name + ": gy differs from the plain kernel"
        assert torch.equal(dgamma, dgamma2) and torch.equal(colsum, colsum2), name + ": sums differ from the plain kernel"
        exact(gy, ref.gy, "scale_residual_bwd_" + name + " gy")
        exact(dgamma, ref.dgamma, "scale_residual_bwd_" + name + " dgamma")
        exact(colsum, ref.colsum, "scale_residual_bwd_" + name + " colsum")


# ------------------------------------------------------------------------------------------------ column sums
def finish_columns(part, d, name):
    """The [256][d] slabs of colsum / gelu_bwd finished as ops does: two halves of d / 2 columns in one launch."""
    nblk, half = LIB().octic_dense_gelu_blocks(), d // 2
    out = Out(1, d)
    ck(LIB().octic_dense_finish(part.ptr, nblk, half, out.ptr, ctypes.c_void_p(out.body.data_ptr() + 4 * half), None, stream()))
    return out.check(name)[0]


@pytest.mark.parametrize("d", COLSUM_WIDTHS)
@pytest.mark.parametrize("rows,rps", COLSUM_ROWS, ids=_id)
def test_colsum_exact(rows, rps, d):
    """octic_dense_colsum and _skip on bf16 integers inside a wider tensor (ld = d + 8, non-zero padding columns, 16
    non-zero rows behind): the finished sums are the integer column sums bit for bit."""
    assert LIB().octic_dense_gelu_blocks() == 256 and 3 * rows < 2 ** 24
    g = _gen(6000 * d + rows)
    ld = d + 8
    t = ints(g, -3, 3, rows, ld)
    t[:, d:] = torch.where(t[:, d:] == 0, torch.ones_like(t[:, d:]), t[:, d:])
    ns = (torch.arange(rows // rps + 2) % 3 != 1).float() / 0.66
    masked = t.clone()
    masked[:rows][(ns[torch.arange(rows) // rps] == 0)] = 0                          # the promise of the mask: dropped rows are zero
    for name, src, mask in (("colsum", t, None), ("colsum_skip", masked, ns), ("colsum of the masked rows", masked, None)):
        gdev = src.to(DEV).bfloat16()
        mdev = mask.to(DEV) if mask is not None else None
        part = Out(256, d)
        if mask is None:
            ck(LIB().octic_dense_colsum(p(gdev), rows, d, ld, part.ptr, stream()))
        else:
            ck(LIB().octic_dense_colsum_skip(p(gdev), rows, d, ld, part.ptr, p(mdev), rps, stream()))
        part.check(name + " partials")
        exact(finish_columns(part, d, name), src[:rows, :d].double().sum(0), name)


# ------------------------------------------------------------------------------------------------------ finish
def test_finish_exact_and_batch():
    """octic_dense_finish at every loop edge of the slab count: out0 only, out1 only, both, out1 with and without scale1,
    bit exact on integer slabs; octic_dense_finish_batch over the same 208 jobs (four launches of mixed widths) is bit
    equal to the single launches."""
    o = O()
    g = _gen(7)
    jobs = []
    for d in FINISH_WIDTHS:
        scale = pick(g, GAMMAS, d)
        for nblk in FINISH_NBLOCKS:
            part = _nonzero_tail(torch.randint(-8, 9, (nblk + TAIL_ROWS, 2, d), generator=g).float(), nblk)
            s0, s1 = part[:nblk, 0].double().sum(0), part[:nblk, 1].double().sum(0)
            pdev, sdev = part.to(DEV), scale.to(DEV)
            for mode in FINISH_MODES:
                want0, want1 = mode in ("out0", "both_scaled"), mode != "out0"
                sc = sdev if mode.endswith("scaled") else None
                name = f"finish d={d} nblocks={nblk} {mode}"
                o0, o1 = finish(pdev, nblk, d, want0, want1, sc, name)
                if want0:
                    exact(o0, s0, name + " out0")
                if want1:
                    exact(o1, s1 * scale.double() if sc is not None else s1, name + " out1")
                jobs.append((name, pdev, nblk, d, sc, o0, o1, Out(1, d) if want0 else None, Out(1, d) if want1 else None))
    arr = (o._FinishJob * len(jobs))()
    for i, (name, pdev, nblk, d, sc, o0, o1, b0, b1) in enumerate(jobs):
        arr[i].partials = pdev.data_ptr()
        arr[i].out0 = b0.body.data_ptr() if b0 else None
        arr[i].out1 = b1.body.data_ptr() if b1 else None
        arr[i].scale1 = sc.data_ptr() if sc is not None else None
        arr[i].nblocks, arr[i].d = nblk, d
    assert len(jobs) == len(FINISH_WIDTHS) * len(FINISH_NBLOCKS) * len(FINISH_MODES) > 3 * 64
    ck(LIB().octic_dense_finish_batch(ctypes.cast(arr, ctypes.c_void_p), len(jobs), stream()))
    for name, pdev, nblk, d, sc, o0, o1, b0, b1 in jobs:
        for single, batch in ((o0, b0), (o1, b1)):
            if batch is not None:
                assert torch.equal(_bits(batch.check(name + " (batch)")[0]), _bits(single)), name + ": batch differs"


# ------------------------------------------------------------------------------------------------ GELU backward
def gelu_grad64(h):
    return 0.5 * (1 + torch.erf(h / math.sqrt(2))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


@pytest.mark.parametrize("d", GELU_WIDTHS)
@pytest.mark.parametrize("rows", GELU_ROWS)
def test_gelu_bwd(rows, d):
    """dh = bf16(gelu'(h) g) within one rounding of float64 (t = the f32 bound 2e-5 (1 + |ref|)); the column sums against
    the float64 sum of the stored dh at rtol 1e-6, atol 2^-22 x the column's sum of |dh|; dh alone with partials = NULL."""
    g = _gen(8000 * d + rows)
    h = (torch.randn(rows + TAIL_ROWS, d, generator=g) * 2).clamp(-6, 6).bfloat16()
    gg = normal(g, rows, d).bfloat16()
    hd, gd = h.to(DEV), gg.to(DEV)
    dh, part = Out(rows, d, BF16), Out(256, d)
    ck(LIB().octic_dense_gelu_bwd(p(hd), p(gd), dh.ptr, part.ptr, rows, d, stream()))
    dh.check("gelu_bwd dh")
    part.check("gelu_bwd partials")
    ref = gelu_grad64(h[:rows].double()) * gg[:rows].double()
    close(dh.body, ref, 2e-5, 2e-5, "gelu_bwd dh", bf16=True)
    stored = dh.body.cpu().double()
    close(finish_columns(part, d, "gelu_bwd column sums"), stored.sum(0), 1e-6, 2.0 ** -22 * stored.abs().sum(0),
          "gelu_bwd column sums")
    dh2 = Out(rows, d, BF16)
    ck(LIB().octic_dense_gelu_bwd(p(hd), p(gd), dh2.ptr, None, rows, d, stream()))
    assert torch.equal(_bits(dh2.check("gelu_bwd dh (no partials)")), _bits(dh.body))
