"""Every kernel instance of csrc/layernorm.hip through the C ABI (ctypes), at every chunk count, layout and row edge, against
the float64 references of tests/golden/ln_d8_cases.py.

Bars (nothing is fixed in advance except the floor):
  f32 outputs   error per element divided by the row's max |reference| (stats: by max(|mean|, spread), rstd: relative);
                the bar of a case is 4 x the error of the oracle (oracle/octic_ref.py LayerNormD8 + autograd) evaluated in
                float32 on the CPU on the same inputs and measured the same way - a wave tree and a sequential sum are both
                O(eps sqrt n) walks that differ by small factors - with a floor of 4 ulp of f32 (4 * 2^-24).
  bf16 y        |got - ref64| <= 1/2 ulp_bf16(ref64) + the f32 bar * row scale: the correct rounding of a correct f32 value.
  dalpha, dbeta the same 4 x rule, each column divided by its sum of |terms|.
  exact         with an integer cotangent in [-8, 8] dbeta is the integer column sum bit for bit; gcast is bit for bit the bf16
                of the scaled dx the same launch wrote; a padded row stride changes no bit.
Every output lies in a NaN-filled arena with guard rows (and, for padded strides, gap columns): after the launch nothing
outside the documented extent may have changed, no NaN may be left inside it, and the inputs are bitwise what they were.

OCTIC_LN_REPORT=<file> writes the measured kernel and oracle errors per route as JSON (the table of NOTES.md).
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import ln_d8_cases as L
from oracle import octic_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2                       # guard rows in front of and behind every arena
F32, BF16 = 0, 1                # dtype codes of include/octic_hip.h
OCTIC_ESHAPE = -1
FLOOR = 4 * 2.0 ** -24
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {torch.float32: F32, torch.bfloat16: BF16}
REPORT = {}                     # (kernel, NV, quantity, input kind) -> [kernel error, oracle error], maxima over the cases


# ------------------------------------------------------------------------------------------------------------- ABI
class LnFinishJob(ctypes.Structure):
    _fields_ = [("partials", ctypes.c_void_p), ("dalpha", ctypes.c_void_p * 5), ("dbeta", ctypes.c_void_p),
                ("nblk", ctypes.c_int), ("c", ctypes.c_int)]


def lib():
    from octic_vits_amd import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _arr5(ts):
    a = (ctypes.c_void_p * 5)()
    for i in range(5):
        a[i] = ts[i].data_ptr() if (ts is not None and ts[i] is not None) else 0
    return a


def _ref(v):
    return ctypes.byref(v) if v is not None else None


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---------------------------------------------------------------------------------------------------------- arenas
class Arena:
    """One allocation of GUARD + rows + GUARD rows of ld elements, NaN everywhere except where `data` goes (the first `width`
    columns of the middle rows: the extent a kernel may read or write)."""

    def __init__(self, rows, width, ld=None, dtype=torch.float32, data=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.buf = torch.full((rows + 2 * GUARD, self.ld), float("nan"), dtype=dtype, device=DEV)
        if data is not None:
            self.body().copy_(data)
        self.snap = self.buf.clone()

    def body(self):
        return self.buf[GUARD:GUARD + self.rows, :self.width]

    def ptr(self, col=0):
        return self.body().data_ptr() + col * self.buf.element_size()

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.snap))

    def outside_untouched(self):
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        m[GUARD:GUARD + self.rows, :self.width] = False
        return torch.equal(_bits(self.buf)[m], _bits(self.snap)[m])

    def filled(self):
        return not bool(torch.isnan(self.body()).any())


class Feature:
    """An octic feature of M rows in one of the four memory layouts.  slot: the operand's number in its call, so that every
    operand (and every tensor of a tuple) gets a row stride of its own under the *_ld layouts."""

    def __init__(self, M, c, dtype, kind, slot, data=None):
        self.c, self.kind = c, kind
        pad = kind.endswith("_ld")
        if kind.startswith("packed"):
            spans = [(0, 8 * c)]
        else:
            spans = [(0, c), (c, c), (2 * c, c), (3 * c, c), (4 * c, 4 * c)]          # the E tensor is [M, 2, 2c]
        self.arenas = [Arena(M, w, w + (8 * (slot + i + 1) if pad else 0), dtype, None if data is None else data[:, lo:lo + w])
                       for i, (lo, w) in enumerate(spans)]

    def view(self):
        from octic_vits_amd._lib import OcticView
        v = OcticView()
        if len(self.arenas) == 1:
            a = self.arenas[0]
            for i in range(5):
                v.ptr[i] = a.ptr(i * self.c)
                v.ld[i] = a.ld
        else:
            for i, a in enumerate(self.arenas):
                v.ptr[i] = a.ptr()
                v.ld[i] = a.ld
        for i in range(5):                                   # what check_view asks of a caller
            assert v.ptr[i] % 16 == 0 and (v.ld[i] * self.arenas[0].buf.element_size()) % 16 == 0
        return v

    def packed(self):
        return torch.cat([a.body() for a in self.arenas], dim=1)

    def unchanged(self):
        return all(a.unchanged() for a in self.arenas)

    def outside_untouched(self):
        return all(a.outside_untouched() for a in self.arenas)

    def filled(self):
        return all(a.filled() for a in self.arenas)


def operand_kind(layout, role):
    """mixed: x is a 5-tuple and every other operand one packed tensor."""
    if layout == "mixed":
        return "tuple" if role == "x" else "packed"
    return layout


# ------------------------------------------------------------------------------------------- references and bars
def _row_err(got, ref):
    """max over rows of max |got - ref| / max |ref| of the row; a row whose reference is all zero must be zero."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d, s = np.abs(got - ref).max(1), np.abs(ref).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(s > 0, d / s, np.where(d > 0, np.inf, 0.0))
    return float(np.nan_to_num(e, nan=np.inf).max())


def _stats_err(mean, rstd, ref):
    mean, rstd = np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    scale = np.maximum(np.abs(ref["mean"]), ref["spread"][:, None])
    e = max(float((np.abs(mean - ref["mean"]) / scale).max()), float((np.abs(rstd - ref["rstd"]) / ref["rstd"]).max()))
    return e if e == e else float("inf")


def _col_err(got5, ref5, scale5):
    e = 0.0
    for g, r, s in zip(got5, ref5, scale5):
        v = float((np.abs(np.asarray(g, np.float64) - r) / s).max())
        e = max(e, v if v == v else float("inf"))
    return e


def _oracle(c, alpha5, beta, dtype):
    """The oracle module with these parameters; unit alpha and zero beta stand in for missing ones (exact in any format)."""
    ln = R.LayerNormD8(8 * c, eps=L.EPS).to(dtype)
    with torch.no_grad():
        for n, i in zip(("A1", "A2", "B1", "B2", "E"), range(5)):
            p = getattr(ln.scaling, "alpha_" + n)
            p.copy_(alpha5[i].to(dtype) if alpha5 is not None else torch.ones_like(p))
        ln.scaling.beta.copy_(beta.to(dtype) if beta is not None else torch.zeros_like(ln.scaling.beta))
    return ln


def _params(c, affine):
    alpha5, beta = L.make_affine(c)
    return (alpha5 if affine != "none" else None), (beta if affine == "alpha_beta" else None)


def _bar(oracle_err):
    return max(4.0 * oracle_err, FLOOR)


@functools.lru_cache(maxsize=None)
def fwd_case(M, c, kind, affine):
    x = L.make_x(M, c, kind)
    alpha5, beta = _params(c, affine)
    y, mean, rstd = L.ln_ref(x.numpy(), alpha5, beta)
    ref = dict(x=x, y=y, mean=mean, rstd=rstd, spread=1.0 / (rstd * L.SQRT2_OVER_4))        # spread = sqrt(S) of the row
    with torch.no_grad():
        u = L.unpack5(x[None], c)
        y32 = L.pack5(_oracle(c, alpha5, beta, torch.float32)(u)).numpy()
        var = lambda t: t.var(dim=-1, unbiased=False)
        S = var(u[0]) + var(u[1]) + var(u[2]) + var(u[3]) + var(u[4]).mean(-1) + L.EPS
        mean32 = torch.cat([t.mean(-1, keepdim=True) for t in u[:4]] + [u[4].mean(-1)], dim=-1)[0].numpy()
        rstd32 = (1.0 / (R.SQRT2_OVER_4 * torch.sqrt(S)))[0].numpy()
    ref["oracle_y"], ref["oracle_stats"] = _row_err(y32, y), _stats_err(mean32, rstd32, ref)
    return ref


@functools.lru_cache(maxsize=None)
def bwd_case(M, c, kind, gd, has_alpha, has_dres, integer_g=False):
    x = L.make_x(M, c, kind)
    g = L.make_int_g(M, c) if integer_g else L.make_g(M, c)
    g = g.to(DT[gd]).float()                                   # the cotangent the kernel sees, exactly
    dres = L.make_g(M, c, "res") if has_dres else None
    alpha5 = L.make_affine(c)[0] if has_alpha else None
    dx, dal, dbeta = L.ln_bwd_ref(g.numpy(), x.numpy(), alpha5, None if dres is None else dres.numpy())
    sal, sbeta = L.param_term_sums(g.numpy(), x.numpy())
    ref = dict(x=x, g=g, dres=dres, dx=dx, dalpha=dal, dbeta=dbeta, sal=sal, sbeta=sbeta)
    ln = _oracle(c, alpha5, None, torch.float32)
    xs = [t.clone().requires_grad_(True) for t in L.unpack5(x[None], c)]
    torch.autograd.backward(ln(tuple(xs)), list(L.unpack5(g[None], c)))
    dx32 = L.pack5([t.grad for t in xs])
    if dres is not None:
        dx32 = dx32 + dres
    ref["oracle_dx"] = _row_err(dx32.numpy(), dx)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref["oracle_dalpha"] = _col_err([getattr(ln.scaling, "alpha_" + n).grad.numpy() for n in ("A1", "A2", "B1", "B2", "E")],
                                        dal, [np.where(s > 0, s, 1.0) for s in sal])
        ref["oracle_dbeta"] = _col_err([ln.scaling.beta.grad.numpy()], [dbeta], [np.where(sbeta > 0, sbeta, 1.0)])
    return ref


def _note(route, quantity, kind, got, oracle):
    k = (route[0], route[1], quantity, "offset1000" if kind == "offset1000" else "well-conditioned")
    r = REPORT.setdefault(k, [0.0, 0.0])
    r[0], r[1] = max(r[0], got), max(r[1], oracle)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("OCTIC_LN_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump([dict(kernel=k[0], NV=k[1], quantity=k[2], inputs=k[3], kernel_err=v[0], oracle_f32_err=v[1])
                       for k, v in sorted(REPORT.items())], f, indent=1)


def _bf16_half_ulp(ref):
    """half the spacing of bfloat16 (8 significant bits) at |ref|; 0 at 0"""
    _, ex = np.frexp(np.abs(ref))
    return np.where(ref != 0, np.ldexp(0.5, ex - 8), 0.0)


# ---------------------------------------------------------------------------------------------------------- launches
def run_fwd(M, c, layout, out_dtype, affine, kind="normal", fails=None, want_stats=True):
    """One forward launch, checked.  Returns (y Feature, stats Arena)."""
    ref = fwd_case(M, c, kind, affine)
    tag = f"fwd c={c} M={M} {layout} {out_dtype} {affine} {kind}"
    alpha5, beta = _params(c, affine)
    alpha_d = [a.to(DEV) for a in alpha5] if alpha5 is not None else None
    beta_d = beta.to(DEV) if beta is not None else None
    xf = Feature(M, c, torch.float32, operand_kind(layout, "x"), 0, ref["x"])
    yf = Feature(M, c, DT[out_dtype], operand_kind(layout, "y"), 1)
    stats = Arena(M, 8)
    xv, yv = xf.view(), yf.view()
    rc = lib().octic_layernorm_d8_fwd(_ref(xv), _ref(yv), _arr5(alpha_d), _p(beta_d), _p(stats.body() if want_stats else None),
                                      M, c, L.EPS, CODE[DT[out_dtype]], _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{tag}: returned {rc}"
    packed = all(operand_kind(layout, r).startswith("packed") for r in "xy")
    route = L.route(c, packed)
    if fails is None:
        return yf, stats
    if not xf.unchanged():
        fails.append(f"{tag}: x changed")
    if alpha_d is not None and not all(torch.equal(a.cpu(), b) for a, b in zip(alpha_d, alpha5)):
        fails.append(f"{tag}: alpha changed")
    if not (yf.outside_untouched() and stats.outside_untouched()):
        fails.append(f"{tag}: a write outside y or stats")
    if not yf.filled():
        fails.append(f"{tag}: {int(torch.isnan(yf.packed()).sum())} elements of y left unwritten (or NaN)")
    if not want_stats:
        if not stats.unchanged():
            fails.append(f"{tag}: stats written although NULL was passed")
        return yf, stats
    if not stats.filled():
        fails.append(f"{tag}: stats left unwritten (or NaN)")
    st = stats.body().double().cpu().numpy()
    if _bits(stats.body()[:, 7].contiguous()).count_nonzero().item():
        fails.append(f"{tag}: stats slot 7 is not +0")
    y = yf.packed().double().cpu().numpy()
    es = _stats_err(st[:, :6], st[:, 6], ref)
    _note(route, "stats", kind, es, ref["oracle_stats"])
    if not es <= _bar(ref["oracle_stats"]):
        fails.append(f"{tag}: stats error {es:.3e} > bar {_bar(ref['oracle_stats']):.3e} (f32 oracle {ref['oracle_stats']:.3e})")
    bar = _bar(ref["oracle_y"])
    if out_dtype == "f32":
        ey = _row_err(y, ref["y"])
        _note(route, "y", kind, ey, ref["oracle_y"])
        if not ey <= bar:
            fails.append(f"{tag}: y error {ey:.3e} > bar {bar:.3e} (f32 oracle {ref['oracle_y']:.3e})")
    else:
        allow = _bf16_half_ulp(ref["y"]) + bar * np.abs(ref["y"]).max(1, keepdims=True)
        over = np.abs(y - ref["y"]) - allow
        if not (over <= 0).all():
            fails.append(f"{tag}: {int((~(over <= 0)).sum())} bf16 elements off by more than half an ulp + the f32 bar, "
                         f"worst by {np.nanmax(over):.3e}")
    return yf, stats


def run_bwd(M, c, layout, gd, has_alpha, has_dres, kind="normal", integer_g=False, fails=None, cast=None, dalpha_bar=True):
    """Forward (for stats), one backward launch and its finish, checked.  cast: (rs tensor or None, rows per scale) sends the
    launch through octic_layernorm_d8_bwd_cast.  Returns dict of the output arenas."""
    ref = bwd_case(M, c, kind, gd, has_alpha, has_dres, integer_g)
    tag = f"bwd c={c} M={M} {layout} g={gd} alpha={has_alpha} dres={has_dres} {kind}{' int' if integer_g else ''}"
    alpha5 = L.make_affine(c)[0] if has_alpha else None
    alpha_d = [a.to(DEV) for a in alpha5] if alpha5 is not None else None
    xf = Feature(M, c, torch.float32, operand_kind(layout, "x"), 0, ref["x"])
    yf = Feature(M, c, torch.float32, operand_kind(layout, "y"), 1)
    st0 = Arena(M, 8)
    xv, yv = xf.view(), yf.view()
    rc = lib().octic_layernorm_d8_fwd(_ref(xv), _ref(yv), _arr5(alpha_d), _p(None), _p(st0.body()), M, c, L.EPS, F32, _stream())
    assert rc == 0, f"{tag}: forward returned {rc}"
    stats = Arena(M, 8, data=st0.body())
    gf = Feature(M, c, DT[gd], operand_kind(layout, "g"), 2, ref["g"])
    rf = Feature(M, c, torch.float32, operand_kind(layout, "dres"), 3, ref["dres"]) if has_dres else None
    df = Feature(M, c, torch.float32, operand_kind(layout, "dx"), 4)
    nblk = lib().octic_layernorm_d8_bwd_blocks(M)
    assert nblk == L.bwd_blocks(M)
    part = Arena(nblk, 16 * c)
    gv, dv, rv = gf.view(), df.view(), (rf.view() if rf is not None else None)
    gcast = None
    if cast is None:
        rc = lib().octic_layernorm_d8_bwd(_ref(gv), _ref(xv), _p(stats.body()), _arr5(alpha_d), _ref(rv), _ref(dv), _p(part.body()),
                                          M, c, CODE[DT[gd]], _stream())
    else:
        gcast = Arena(M, 8 * c, dtype=torch.bfloat16)
        rc = lib().octic_layernorm_d8_bwd_cast(_ref(gv), _ref(xv), _p(stats.body()), _arr5(alpha_d), _ref(rv), _ref(dv),
                                               _p(part.body()), M, c, _p(cast[0]), cast[1], _p(gcast.body()), _stream())
    torch.cuda.synchronize()
    out = dict(rc=rc, dx=df, partials=part, gcast=gcast, stats=stats, inputs=[xf, gf, stats] + ([rf] if rf is not None else []))
    if rc != 0:
        return out
    dal = [Arena(1, c if i < 4 else 2 * c) for i in range(5)]
    dbeta = Arena(1, c)
    rc2 = lib().octic_layernorm_d8_bwd_finish(_p(part.body()), nblk, c, _arr5([a.body() for a in dal]), _p(dbeta.body()), _stream())
    torch.cuda.synchronize()
    assert rc2 == 0, f"{tag}: finish returned {rc2}"
    out.update(dalpha=dal, dbeta=dbeta)
    if fails is None:
        return out
    packed = all(operand_kind(layout, r).startswith("packed") for r in ("x", "g", "dres", "dx"))
    route = L.route(c, packed, gd, cast=cast is not None)
    if not all(f.unchanged() for f in out["inputs"]):
        fails.append(f"{tag}: an input changed")
    if not (df.outside_untouched() and part.outside_untouched() and dbeta.outside_untouched()
            and all(a.outside_untouched() for a in dal) and (gcast is None or gcast.outside_untouched())):
        fails.append(f"{tag}: a write outside dx, gcast, partials, dalpha or dbeta")
    if not (df.filled() and dbeta.filled() and all(a.filled() for a in dal) and (gcast is None or gcast.filled())):
        fails.append(f"{tag}: {int(torch.isnan(df.packed()).sum())} elements of dx left unwritten (or NaN), or NaN in "
                     "dalpha / dbeta / gcast")
    got_beta = dbeta.body()[0].double().cpu().numpy()
    if integer_g:
        # plane 1 of the slabs and its reduction tree, exactly: a dropped or doubled row, wave or slab cannot hide
        if not np.array_equal(got_beta, ref["dbeta"]):
            fails.append(f"{tag}: dbeta is not the integer column sum in {int((got_beta != ref['dbeta']).sum())} of {c} columns")
        return out
    e = _row_err(df.packed().double().cpu().numpy(), ref["dx"])
    _note(route, "dx", kind, e, ref["oracle_dx"])
    if not e <= _bar(ref["oracle_dx"]):
        fails.append(f"{tag}: dx error {e:.3e} > bar {_bar(ref['oracle_dx']):.3e} (f32 oracle {ref['oracle_dx']:.3e})")
    with np.errstate(divide="ignore", invalid="ignore"):
        e = _col_err([a.body()[0].double().cpu().numpy() for a in dal], ref["dalpha"], [np.where(s > 0, s, 1.0) for s in ref["sal"]])
        _note(route, "dalpha", kind, e, ref["oracle_dalpha"])
        if dalpha_bar and not e <= _bar(ref["oracle_dalpha"]):
            fails.append(f"{tag}: dalpha error {e:.3e} > bar {_bar(ref['oracle_dalpha']):.3e} (f32 oracle {ref['oracle_dalpha']:.3e})")
        e = _col_err([got_beta], [ref["dbeta"]], [np.where(ref["sbeta"] > 0, ref["sbeta"], 1.0)])
        _note(route, "dbeta", kind, e, ref["oracle_dbeta"])
        if not e <= _bar(ref["oracle_dbeta"]):
            fails.append(f"{tag}: dbeta error {e:.3e} > bar {_bar(ref['oracle_dbeta']):.3e} (f32 oracle {ref['oracle_dbeta']:.3e})")
    return out


def _done(fails):
    for f in fails:
        print(f)
    assert not fails, f"{len(fails)} checks failed, the first: " + " | ".join(fails[:5])


LAYOUT_C = [(layout, c) for layout in L.LAYOUTS for c in L.matrix_c(layout)]


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("layout,c", LAYOUT_C)
def test_forward(layout, c):
    """Every forward instance at every small row count: y and stats against float64, stats slot 7 = +0, arenas."""
    fails = []
    for M in L.SMALL_M:
        for out_dtype in ("f32", "bf16"):
            for affine in L.AFFINE:
                for kind in (L.KINDS if M == 9 else ["normal"]):
                    run_fwd(M, c, layout, out_dtype, affine, kind, fails)
    run_fwd(9, c, layout, "bf16", "alpha_beta", fails=fails, want_stats=False)
    _done(fails)


@pytest.mark.parametrize("layout,c", LAYOUT_C)
def test_backward(layout, c):
    """Every backward instance at every small row count: dx and dbeta against float64, dbeta exactly with an integer
    cotangent, arenas.  (The bar of dalpha has a test of its own below, one case per row count.)"""
    fails = []
    for M in L.SMALL_M:
        for gd in ("f32", "bf16"):
            for has_alpha in (True, False):
                for has_dres in (True, False):
                    for kind in (L.KINDS if (M == 9 and has_alpha and has_dres) else ["normal"]):
                        run_bwd(M, c, layout, gd, has_alpha, has_dres, kind, fails=fails, dalpha_bar=False)
            run_bwd(M, c, layout, gd, True, True, integer_g=True, fails=fails)
    _done(fails)


_DALPHA_ONE_ROW = pytest.mark.xfail(strict=True, reason="one row, c = 192: dalpha error 6.64e-05 > 4 x the f32 oracle's 6.08e-06; "
                                    "the f32 mean's rounding over a column 8.2e-4 from the mean, see test_backward_dalpha")


@pytest.mark.parametrize("layout,c,M", [pytest.param(layout, c, M, marks=[_DALPHA_ONE_ROW] if (c, M) == (192, 1) else [])
                                        for layout, c in LAYOUT_C for M in L.SMALL_M])
def test_backward_dalpha(layout, c, M):
    """dalpha of every backward instance within 4 x the f32 oracle's error, each column divided by its sum of |terms|.

    Known to fail, and kept failing (strict xfail), at c = 192, M = 1 (packed and packed_ld).  One row makes every dalpha column
    a single term g * (x - mean) * rstd, whose relative error is the error of the f32 mean over |x - mean| of that column.  The
    seeded row has a B1 column 8.2e-4 from its segment mean; the kernel's mean is 0.92 ulp = 5.5e-8 off there (a correctly
    rounded f32 mean is up to 0.5 ulp off) and the column's error is 6.64e-05 against the oracle's 6.08e-06 (bar 2.43e-05) for
    an f32 cotangent, 6.63e-05 against 5.99e-06 (bar 2.40e-05) for a bf16 one, in every combination of alpha and dres.
    Replaying the lane-group arithmetic in numpy float32 gives 6.65e-05 whether the mean is s * (1 / n) as in the kernel or
    s / n: no f32 mean does better by rule, and on the same measure the oracle itself has 2.3e-04 at c = 224 where the kernel
    has 1.1e-05.  Nothing to fix in the kernel was found."""
    fails = []
    for gd in ("f32", "bf16"):
        for has_alpha in (True, False):
            for has_dres in (True, False):
                for kind in (L.KINDS if (M == 9 and has_alpha and has_dres) else ["normal"]):
                    run_bwd(M, c, layout, gd, has_alpha, has_dres, kind, fails=fails)
    _done([f for f in fails if "dalpha error" in f])


@pytest.mark.parametrize("M", L.FWD_STRIDE_M)
@pytest.mark.parametrize("layout,c", [("packed", 32), ("packed", 8), ("tuple", 8)])
def test_forward_grid_stride_edge(layout, c, M):
    """4096 blocks x 4 waves: the last M whose rows all have a wave of their own and the first that sends a wave round again."""
    fails = []
    for out_dtype in ("f32", "bf16"):
        run_fwd(M, c, layout, out_dtype, "alpha_beta", fails=fails)
    _done(fails)


@pytest.mark.parametrize("M", L.BWD_STRIDE_M)
@pytest.mark.parametrize("layout,c,gd", [("packed", 32, "f32"), ("packed", 32, "bf16"), ("packed", 192, "bf16"),
                                         ("packed", 8, "f32"), ("packed", 8, "bf16"), ("tuple", 8, "f32"), ("tuple", 8, "bf16")])
def test_backward_grid_stride_edge(layout, c, gd, M):
    """256 blocks x 8 waves, each family at its smallest c (the narrow bf16 kernel starts at c = 192)."""
    fails = []
    run_bwd(M, c, layout, gd, True, True, fails=fails)
    run_bwd(M, c, layout, gd, True, True, integer_g=True, fails=fails)
    _done(fails)


@pytest.mark.parametrize("c", L.G8_C + L.GENERIC_C)
def test_padded_row_stride_changes_no_bit(c):
    """packed_ld runs the kernel packed runs (same c, dtype, NV): every output is bitwise the same."""
    M = 33
    for out_dtype in ("f32", "bf16"):
        (ya, sa), (yb, sb) = (run_fwd(M, c, lay, out_dtype, "alpha_beta") for lay in ("packed", "packed_ld"))
        assert torch.equal(_bits(ya.packed()), _bits(yb.packed())), f"y {out_dtype}"
        assert torch.equal(_bits(sa.body()), _bits(sb.body())), f"stats {out_dtype}"
    for gd in ("f32", "bf16"):
        a, b = (run_bwd(M, c, lay, gd, True, True) for lay in ("packed", "packed_ld"))
        assert torch.equal(_bits(a["dx"].packed()), _bits(b["dx"].packed())), f"dx {gd}"
        for p, q in zip(a["dalpha"] + [a["dbeta"]], b["dalpha"] + [b["dbeta"]]):
            assert torch.equal(_bits(p.body()), _bits(q.body())), f"dalpha / dbeta {gd}"


@pytest.mark.parametrize("layout", ["packed", "packed_ld"])
@pytest.mark.parametrize("c", L.CAST_C)
def test_gcast_is_the_bf16_of_the_scaled_dx(c, layout):
    """octic_layernorm_d8_bwd_cast: gcast = bf16(rs[row // rps] * dx) of the dx the same launch wrote, bit for bit; dx and the
    parameter gradients are those of the plain call."""
    B, T = 3, 11
    M = B * T
    per_row = (0.5 + 0.03125 * torch.arange(M, dtype=torch.float32)).to(DEV)          # a different factor in every row
    variants = {"NULL": (None, 1), "rps=1": (per_row, 1), "rps=T": (torch.tensor([1.5, 0.75, 1.25], device=DEV), T),
                "zero": (torch.tensor([1.5, 0.0, 0.75], device=DEV), T)}
    fails = []
    for has_dres in (True, False):
        plain = run_bwd(M, c, layout, "bf16", True, has_dres)
        for name, (rs, rps) in variants.items():
            out = run_bwd(M, c, layout, "bf16", True, has_dres, fails=fails, cast=(rs, rps))
            assert out["rc"] == 0, f"{name}: returned {out['rc']}"
            dx = out["dx"].packed()
            scale = rs[torch.arange(M, device=DEV) // rps] if rs is not None else torch.ones(M, device=DEV)
            want = (dx * scale[:, None]).to(torch.bfloat16)
            if not torch.equal(_bits(out["gcast"].body().contiguous()), _bits(want)):
                fails.append(f"c={c} {name} dres={has_dres}: gcast differs in {int((_bits(out['gcast'].body().contiguous()) != _bits(want)).sum())} elements")
            same = torch.equal(_bits(dx), _bits(plain["dx"].packed())) and all(
                torch.equal(_bits(p.body()), _bits(q.body()))
                for p, q in zip(out["dalpha"] + [out["dbeta"]], plain["dalpha"] + [plain["dbeta"]]))
            if not same:
                fails.append(f"c={c} {name} dres={has_dres}: dx / dalpha / dbeta differ from the plain call")
    _done(fails)


@pytest.mark.parametrize("layout,c", L.CAST_REFUSED)
def test_bwd_cast_refuses_and_writes_nothing(layout, c):
    """c = 192 (the narrow kernel), c = 48 (no lane-group kernel) and a tuple view: OCTIC_ESHAPE, not a byte written."""
    out = run_bwd(9, c, layout, "bf16", True, True, cast=(None, 1))
    assert out["rc"] == OCTIC_ESHAPE
    assert out["dx"].unchanged() and out["gcast"].unchanged() and out["partials"].unchanged()
    assert all(f.unchanged() for f in out["inputs"])


# ---------------------------------------------------------------------------------------------------------- finish
def _partials(nblk, c, integer, seed):
    """[nblk, 2, 8c] the way the backward kernels leave it: plane 0 whole, plane 1 in its first c columns; the rest NaN, which
    the reduction therefore must not read."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * nblk + c)
    p = torch.full((nblk, 2, 8 * c), float("nan"))
    if integer:
        p[:, 0] = torch.randint(-8, 9, (nblk, 8 * c), generator=gen).float()
        p[:, 1, :c] = torch.randint(-8, 9, (nblk, c), generator=gen).float()
    else:
        p[:, 0] = torch.randn(nblk, 8 * c, generator=gen)
        p[:, 1, :c] = torch.randn(nblk, c, generator=gen)
    return p


def _finish_terms(p, c):
    """per output tensor, the float64 terms [n, columns] the reduction adds"""
    p = p.double().numpy()
    return [p[:, 0, i * c:(i + 1) * c] for i in range(4)] + [np.concatenate([p[:, 0, 4 * c:6 * c], p[:, 0, 6 * c:8 * c]], 0), p[:, 1, :c]]


def _finish(p, c, present=(True,) * 6):
    nblk = p.shape[0]
    part = Arena(nblk, 16 * c, data=p.reshape(nblk, 16 * c))
    outs = [Arena(1, c if i != 4 else 2 * c) for i in range(6)]                      # dalpha A1..B2, dalpha_E, dbeta
    rc = lib().octic_layernorm_d8_bwd_finish(_p(part.body()), nblk, c, _arr5([outs[i].body() if present[i] else None for i in range(5)]),
                                             _p(outs[5].body() if present[5] else None), _stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert part.unchanged(), "partials changed"
    for i, a in enumerate(outs):
        assert a.outside_untouched(), f"a write outside output {i}"
        assert a.filled() if present[i] else a.unchanged(), f"output {i}: {'NaN left' if present[i] else 'written although NULL'}"
    return outs


@pytest.mark.parametrize("c", L.FINISH_C)
@pytest.mark.parametrize("nblk", L.FINISH_NBLK)
def test_finish_sums_every_slab_once(nblk, c):
    """Integer slabs: the five dalpha (E = both E planes) and dbeta are the integer sums bit for bit.  Random slabs: within
    n * 2^-24 * sum |terms| of the float64 sum, n the number of terms - the bound of an f32 sum of n terms in any order."""
    p = _partials(nblk, c, True, 1)
    for i, (a, t) in enumerate(zip(_finish(p, c), _finish_terms(p, c))):
        assert np.array_equal(a.body()[0].double().cpu().numpy(), t.sum(0)), f"integer sum of output {i}"
    p = _partials(nblk, c, False, 2)
    for i, (a, t) in enumerate(zip(_finish(p, c), _finish_terms(p, c))):
        err = np.abs(a.body()[0].double().cpu().numpy() - t.sum(0))
        assert (err <= t.shape[0] * 2.0 ** -24 * np.abs(t).sum(0)).all(), f"output {i}: {err.max():.3e}"


@pytest.mark.parametrize("c", L.FINISH_C)
def test_finish_with_a_null_output(c):
    p = _partials(49, c, False, 3)
    full = _finish(p, c)
    for k in range(6):
        outs = _finish(p, c, tuple(i != k for i in range(6)))
        for i in range(6):
            if i != k:
                assert torch.equal(_bits(outs[i].body()), _bits(full[i].body())), f"output {i} with output {k} NULL"


def test_finish_batch_equals_single_calls():
    """50 jobs (two launches of at most 48) of four different c and thirteen different slab counts, every seventh without
    dbeta and every fifth without one of its dalpha."""
    jobs = (LnFinishJob * L.BATCH_JOBS)()
    keep, single = [], []
    for j in range(L.BATCH_JOBS):
        c, nblk = L.BATCH_C[j % len(L.BATCH_C)], L.FINISH_NBLK[j % len(L.FINISH_NBLK)]
        p = _partials(nblk, c, False, 100 + j)
        present = tuple(not ((i == 5 and j % 7 == 3) or (j % 5 == 2 and i == (j // 5) % 5)) for i in range(6))
        single.append(_finish(p, c, present))
        part = Arena(nblk, 16 * c, data=p.reshape(nblk, 16 * c))
        outs = [Arena(1, c if i != 4 else 2 * c) for i in range(6)]
        keep.append((part, outs))
        jobs[j].partials = part.ptr()
        for i in range(5):
            jobs[j].dalpha[i] = outs[i].ptr() if present[i] else 0
        jobs[j].dbeta, jobs[j].nblk, jobs[j].c = (outs[5].ptr() if present[5] else 0), nblk, c
    assert lib().octic_layernorm_d8_bwd_finish_batch(ctypes.cast(jobs, ctypes.c_void_p), 0, _stream()) == 0
    torch.cuda.synchronize()
    assert all(a.unchanged() for _, outs in keep for a in outs), "njobs = 0 wrote something"
    assert lib().octic_layernorm_d8_bwd_finish_batch(ctypes.cast(jobs, ctypes.c_void_p), L.BATCH_JOBS, _stream()) == 0
    torch.cuda.synchronize()
    for j, ((part, outs), want) in enumerate(zip(keep, single)):
        assert part.unchanged()
        for i in range(6):
            assert outs[i].outside_untouched(), f"job {j}: a write outside output {i}"
            # (an output passed as NULL stays NaN in both: the comparison then says that neither call wrote it)
            assert torch.equal(_bits(outs[i].body()), _bits(want[i].body())), f"job {j} (c = {jobs[j].c}, nblk = {jobs[j].nblk}) output {i}"
