"""MaxFiltering / Canonization kernels (csrc/orbit_invariant.hip) against float64, through the C ABI and through the modules.

Exact cases: small-integer operands make every dot exact in bf16 operands and f32 sums, so out, idx, dx, dref and the
canonized rows are compared bit for bit with float64 (rounded once to the stored dtype).  The shapes cover c in {8, 24, 40, 160},
R in {1, 24, 40, 130} and M in {1, 70, 257, 1793}, each value at least once (257: two row slabs of 160 rows in the reference
gradient, the last 32-row chunk holding one row; 1793 = 7 x 256 + 1: eight slabs of 256 rows, one row past a slab edge - the
test asks the plan), in both dtypes, on packed and row-strided views, with NaN rows behind row M - 1 and guard
bands around every output and the workspace.
Random cases: the float64 oracle runs on the operands rounded to the compute dtype; bounds are the f32 summation bounds
(n + 2) 2^-24 sum |a| |b| for n terms in any order, plus half an ulp of the stored dtype where the result is stored rounded
(out, and dx which the kernel stores in the compute dtype).
"""
import ctypes

import pytest
import torch

from octic_vits_amd import _lib, ops
from octic_vits_amd import d8_invariantization as INV
from octic_vits_amd import functional as OF
from octic_vits_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
SLOT = (0, 1, 2, 3, 4, 6, 5, 7)            # packed column block -> 8-tuple component


def _mats():
    return torch.stack(INV._orbit_matrices()).double()


def _pack(x8):                               # [M, 8, c] component-major -> packed rows [M, 8c]
    return torch.cat([x8[:, j] for j in SLOT], dim=-1)


def _unpack(xp, c):                          # packed rows -> [M, 8, c]
    M = xp.shape[0]
    blocks = xp.view(M, 8, c)
    out = torch.empty_like(blocks)
    for s, j in enumerate(SLOT):
        out[:, j] = blocks[:, s]
    return out


def _first_max(prod):                        # lowest index among the maxima along dim 1
    mx = prod.max(dim=1, keepdim=True).values
    ar = torch.arange(prod.shape[1]).view(1, -1, *([1] * (prod.dim() - 2)))
    return torch.where(prod == mx, ar, 8).min(dim=1).values


def oracle_max_filter(x8, ref, g=None, idx=None):
    """float64 on CPU.  x8 [M, 8, c], ref [R, c, 8], g [M, R] -> prod [M, 8, R], idx, dx [M, 8, c], dref [R, c, 8]."""
    mats = _mats()
    rexp = torch.einsum("gij,dcj->gdic", mats, ref)                       # [8, R, 8, c]
    prod = torch.einsum("tic,gdic->tgd", x8, rexp)
    if idx is None:
        idx = _first_max(prod)
    if g is None:
        return prod, idx, None, None
    W = torch.zeros_like(prod).scatter_(1, idx.unsqueeze(1), g.unsqueeze(1))
    dx = torch.einsum("tgd,gdic->tic", W, rexp)
    dref = torch.einsum("tgd,gij,tic->dcj", W, mats, x8)
    return prod, idx, dx, dref


def oracle_canonize(x8, refv, c):
    mats = _mats()
    orbit = torch.einsum("gij,tjc->tgic", mats, x8)                       # [M, 8, 8, c]
    dots = torch.einsum("tgic,ic->tg", orbit, refv.view(8, c))
    idx = _first_max(dots)
    out = orbit[torch.arange(x8.shape[0]), idx].flatten(1)
    return dots, idx, out


class Guarded:
    """n elements of dtype inside a buffer with 64-element sentinel bands on both sides."""
    BAND = 64

    def __init__(self, n, dtype, fill=None):
        self.sent = 77 if dtype == torch.uint8 else -12345.0
        self.buf = torch.full((n + 2 * self.BAND,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[self.BAND:self.BAND + n]
        if fill is not None:
            self.t.fill_(fill)

    def ok(self):
        return bool((self.buf[:self.BAND] == self.sent).all() and (self.buf[-self.BAND:] == self.sent).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _x_view(xp, c, layout, pad_rows=3):
    """Device copy of packed rows xp [M, 8c] as a packed or row-strided view, with NaN rows behind row M - 1."""
    M = xp.shape[0]
    ld = 8 * c + (8 if layout == "strided" else 0)
    buf = torch.full((M + pad_rows, ld), float("nan"), dtype=xp.dtype, device=DEV)
    buf[:M, :8 * c] = xp.to(DEV)
    return buf[:M, :8 * c], buf


def run_max_filter(xp, ref, g, c, dt, layout, out_dt=None):
    """All four launches through the C ABI on guarded buffers.  xp packed [M, 8c], ref [R, c, 8] f32, g [M, R] (all CPU, already
    representable in dt).  Returns out, idx, dx (packed), dref on the CPU."""
    L = lib()
    M, R = xp.shape[0], ref.shape[0]
    out_dt = out_dt or dt
    code, ocode = ops.dt_code(dt), ops.dt_code(out_dt)
    xv_t, keep = _x_view(xp.to(dt), c, layout)
    xv = ops._orbit_view(xv_t, c)
    planes = Guarded(8 * R * c, dt)
    _lib.check(L.octic_max_filter_prep(_p(ref.to(DEV).contiguous()), _p(planes.t), R, c, code, _stream()))
    out, idx = Guarded(M * R, out_dt), Guarded(M * R, torch.uint8)
    _lib.check(L.octic_max_filter_fwd(ctypes.byref(xv), _p(planes.t), _p(out.t), _p(idx.t), M, R, c, code, ocode, _stream()))
    gd = g.to(dt).to(DEV).contiguous()
    dx = Guarded(M * 8 * c, dt)
    dv = ops.pview(dx.t.view(M, 8 * c), c)
    _lib.check(L.octic_max_filter_bwd_x(_p(gd), _p(idx.t), _p(planes.t), ctypes.byref(dv), M, R, c, code, _stream()))
    need = int(L.octic_max_filter_bwd_ref_workspace_bytes(M, R, c))
    ws, dref = Guarded(need // 4, torch.float32), Guarded(R * c * 8, torch.float32)
    _lib.check(L.octic_max_filter_bwd_ref(_p(gd), _p(idx.t), ctypes.byref(xv), _p(dref.t), _p(ws.t), need, M, R, c, code, _stream()))
    torch.cuda.synchronize()
    for name, gb in (("planes", planes), ("out", out), ("idx", idx), ("dx", dx), ("workspace", ws), ("dref", dref)):
        assert gb.ok(), f"{name}: guard band overwritten"
    assert torch.isnan(keep[M:]).all()
    return (out.t.view(M, R).cpu(), idx.t.view(M, R).cpu().long(), dx.t.view(M, 8 * c).cpu(), dref.t.view(R, c, 8).cpu())


def run_canonize(xp, refv, g, c, dt, layout, out_dt=None):
    L = lib()
    M = xp.shape[0]
    out_dt = out_dt or dt
    code, ocode = ops.dt_code(dt), ops.dt_code(out_dt)
    xv_t, keep = _x_view(xp.to(dt), c, layout)
    xv = ops._orbit_view(xv_t, c)
    out, idx = Guarded(M * 8 * c, out_dt), Guarded(M, torch.uint8)
    _lib.check(L.octic_canonize_fwd(ctypes.byref(xv), _p(refv.float().to(DEV)), _p(out.t), _p(idx.t), M, c, code, ocode, _stream()))
    gd = g.to(out_dt).to(DEV).contiguous()
    dx = Guarded(M * 8 * c, dt)
    dv = ops.pview(dx.t.view(M, 8 * c), c)
    _lib.check(L.octic_canonize_bwd(_p(gd), ocode, _p(idx.t), ctypes.byref(dv), M, c, code, _stream()))
    torch.cuda.synchronize()
    assert out.ok() and idx.ok() and dx.ok()
    return out.t.view(M, 8 * c).cpu(), idx.t.cpu().long(), dx.t.view(M, 8 * c).cpu()


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).double()


def _same(a, b):
    return torch.equal(a.double(), b.double())


EXACT = [(1, 8, 1), (70, 24, 24), (257, 40, 40), (1793, 8, 130), (70, 160, 130), (257, 160, 24)]


@pytest.mark.parametrize("layout", ["packed", "strided"])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("M,c,R", EXACT)
def test_max_filter_exact(M, c, R, dtn, layout):
    dt = DT[dtn]
    if M == 1793:                                # one row past a row-slab edge of the reference gradient
        slabs, slab_rows = ops.max_filter_bwd_ref_plan(M, R, c)[:2]
        assert slabs > 1 and (M - 1) % slab_rows == 0 and (slabs - 1) * slab_rows + 1 == M
    gen = torch.Generator().manual_seed(1000 * M + 10 * c + R)
    x8, ref, g = _ints((M, 8, c), -3, 3, gen), _ints((R, c, 8), -2, 2, gen), _ints((M, R), -2, 2, gen)
    prod, idx, dx, dref = oracle_max_filter(x8, ref, g)
    out_g, idx_g, dx_g, dref_g = run_max_filter(_pack(x8), ref.float(), g, c, dt, layout)
    assert torch.equal(idx_g, idx), "idx (lowest index among equal products)"
    assert _same(out_g, prod.max(dim=1).values.to(dt)), "out"
    assert _same(dx_g, _pack(dx).to(dt)), "dx"
    assert _same(dref_g, dref.float()), "dref"
    if M > 1 and R > 1:                          # small integers tie often: the rule is exercised, not only planted below
        top = prod.max(dim=1, keepdim=True).values
        assert ((prod == top).sum(1) > 1).any()


def _act(g, v8):                                 # A_g v for v [.., 8, c]
    return torch.einsum("ij,...jc->...ic", _mats()[g], v8)


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_max_filter_planted_ties_and_every_winner(dtn):
    """Row p < 28 is A_a r_p + A_b r_p for the p-th pair a < b of group elements: elements a and b tie for the maximum against
    reference p, and the lower index must win.  Row 28 + g is A_g r_0: element g wins against reference 0, so all 8 signed
    permutations and their transposes (dx, dref) are used."""
    c, R = 8, 40
    gen = torch.Generator().manual_seed(5)
    ref = _ints((R, c, 8), -2, 2, gen)
    r8 = ref.permute(0, 2, 1)                    # [R, 8, c]
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)]
    rows = [_act(a, r8[p]) + _act(b, r8[p]) for p, (a, b) in enumerate(pairs)] + [_act(g, r8[0]) for g in range(8)]
    x8 = torch.stack(rows)
    M = x8.shape[0]
    g = _ints((M, R), -2, 2, gen)
    prod, idx, dx, dref = oracle_max_filter(x8, ref, g)
    for p, (a, b) in enumerate(pairs):
        col = prod[p, :, p]
        assert col[a] == col[b] == col.max() and idx[p, p] <= a, (a, b)
    assert [int(idx[28 + k, 0]) for k in range(8)] == list(range(8))
    out_g, idx_g, dx_g, dref_g = run_max_filter(_pack(x8), ref.float(), g, c, DT[dtn], "packed")
    assert torch.equal(idx_g, idx)
    assert _same(out_g, prod.max(dim=1).values.to(DT[dtn])) and _same(dx_g, _pack(dx).to(DT[dtn])) and _same(dref_g, dref.float())


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_nan_products_win_first(dtn):
    """Row 0: a NaN component makes all 8 products NaN -> winner 0.  Row 1: x0 = x1 = inf against positive reference entries:
    the products of e .. rrr are +inf, those of m .. mrrr are inf - inf = NaN -> the first NaN, element 4 (as torch.max)."""
    c, R, dt = 8, 24, DT[dtn]
    gen = torch.Generator().manual_seed(6)
    ref = _ints((R, c, 8), -2, 2, gen)
    ref[:, 0, 0] = 1
    ref[:, 0, 1] = 1
    x8 = _ints((3, 8, c), -3, 3, gen)
    x8[0, 4, 3] = float("nan")
    x8[1] = 0
    x8[1, 0, 0] = x8[1, 1, 0] = float("inf")
    xp = _pack(x8).to(dt)
    out, idx = ops.max_filter_fwd(xp.to(DEV), ops.max_filter_prep(ref.float().to(DEV), dt), c, dt)
    want = torch.einsum("tic,gdic->tgd", x8, torch.einsum("gij,dcj->gdic", _mats(), ref)).max(dim=1)
    assert torch.isnan(out[:2]).all() and (idx[0] == 0).all() and (idx[1] == 4).all()
    assert torch.isnan(want.values[:2]).all() and (want.indices[0] == 0).all() and (want.indices[1] == 4).all()
    assert _same(out[2].cpu(), want.values[2].to(dt))
    refv = _ints((8 * c,), 1, 2, gen)
    o, i = ops.canonize_fwd(xp.to(DEV), refv.float().to(DEV), c, dt)
    assert torch.isnan(o[0]).any() and int(i[0]) == 0 and int(i[1]) == 4


@pytest.mark.parametrize("layout", ["packed", "strided"])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("M,c", [(1, 8), (70, 24), (257, 40), (70, 160)])
def test_canonize_exact(M, c, dtn, layout):
    dt = DT[dtn]
    gen = torch.Generator().manual_seed(7 * M + c)
    refv = _ints((8 * c,), -2, 2, gen)
    x8 = _ints((M, 8, c), -3, 3, gen)
    n = min(8, M)
    x8[:n] = torch.stack([_act(g, refv.view(8, c)) for g in range(8)])[:n]     # A_g' x = reference for g' = g^-1: every winner
    g = _ints((M, 8 * c), -2, 2, gen)
    dots, idx, out = oracle_canonize(x8, refv, c)
    if M >= 8:
        assert set(idx[:8].tolist()) == set(range(8))
    mats = _mats()
    dx = torch.einsum("tij,tic->tjc", mats[idx], g.view(M, 8, c))                # the transposed (= inverse) signed permutation
    out_g, idx_g, dx_g = run_canonize(_pack(x8), refv, g, c, dt, layout)
    assert torch.equal(idx_g, idx)
    assert _same(out_g, out) and _same(dx_g, _pack(dx))


# ------------------------------------------------------------------------------------------ random operands
def _rounded(t, dt):
    return t.to(dt).double()


def _half_ulp(v, dt):
    if dt == torch.float32:
        return torch.zeros_like(v)
    return torch.maximum(v.abs(), torch.tensor(2.0 ** -126, dtype=v.dtype)).log2().floor().exp2() * 2.0 ** -8


RANDOM = [(70, 24, 40), (257, 16, 72), (130, 40, 96)]


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("M,c,R", RANDOM)
def test_max_filter_random(M, c, R, dtn, seed):
    dt = DT[dtn]
    torch.manual_seed(seed)
    mod = INV.MaxFilteringInvariant(8 * c, num_references=R)
    ref32 = mod.references.detach()
    ref, x8 = _rounded(ref32, dt), _rounded(torch.randn(M, 8, c), dt)
    g = _rounded(torch.randn(M, R), dt)
    eps = 2.0 ** -24
    prod, idx0, _, _ = oracle_max_filter(x8, ref)
    ax, ar = x8.abs(), ref.abs()
    amats = _mats().abs()
    mag = torch.einsum("tic,gdic->tgd", ax, torch.einsum("gij,dcj->gdic", amats, ar)).max(dim=1).values   # max_g sum |A_g||x||ref|
    bound = (8 * c + 8) * eps * mag                                              # per product, [M, R]
    top2 = prod.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) <= 2 * bound
    frac = near.double().mean().item()
    print(f"near ties: {100 * frac:.3f} % of {M * R} pairs")
    assert frac <= 0.005
    g = torch.where(near, torch.zeros_like(g), g)                                # gradients do not depend on a near tie's choice
    out_g, idx_g, dx_g, dref_g = run_max_filter(_pack(x8), ref32, g, c, dt, "packed")
    assert torch.equal(idx_g[~near], idx0[~near])
    best = prod.max(dim=1).values
    chosen = prod.gather(1, idx_g.unsqueeze(1)).squeeze(1)
    assert ((best - chosen) <= 2 * bound).all(), "a near tie's winner is not a candidate within the bound"
    err = (out_g.double() - best).abs()
    tol = bound + _half_ulp(best, dt)
    print(f"out: max err / bound {(err / tol).max().item():.3f}")
    assert (err <= tol).all()
    _, _, dx, dref = oracle_max_filter(x8, ref, g, idx=idx_g)
    rsel = torch.einsum("gij,dcj->gdic", amats, ar)                              # |A_g| |ref|
    Wabs = torch.zeros_like(prod).scatter_(1, idx_g.unsqueeze(1), g.abs().unsqueeze(1))
    dx_mag = torch.einsum("tgd,gdic->tic", Wabs, rsel)
    dx_tol = _pack((2 * R + 2) * eps * dx_mag) + _half_ulp(_pack(dx), dt)
    dx_err = (dx_g.double() - _pack(dx)).abs()
    print(f"dx: max err / bound {(dx_err / dx_tol.clamp_min(1e-300)).max().item():.3f}")
    assert (dx_err <= dx_tol).all()
    slabs = ops.max_filter_bwd_ref_plan(M, R, c)[0]
    dref_mag = torch.einsum("tgd,gij,tic->dcj", Wabs, amats, ax)
    dref_tol = (2 * M + 2 + slabs) * eps * dref_mag
    dref_err = (dref_g.double() - dref).abs()
    print(f"dref: max err / bound {(dref_err / dref_tol.clamp_min(1e-300)).max().item():.3f}")
    assert (dref_err <= dref_tol).all()


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("M,c", [(70, 24), (257, 16), (130, 40)])
def test_canonize_random(M, c, dtn):
    dt = DT[dtn]
    torch.manual_seed(M)
    mod = INV.CanonizationInvariant(8 * c)
    refv, x8 = _rounded(mod.reference.detach(), dt), _rounded(torch.randn(M, 8, c), dt)
    dots, idx0, _ = oracle_canonize(x8, refv, c)
    mag = torch.einsum("tgic,ic->tg", torch.einsum("gij,tjc->tgic", _mats().abs(), x8.abs()), refv.abs().view(8, c)).max(1).values
    bound = (8 * c + 8) * 2.0 ** -24 * mag
    top2 = dots.topk(2, dim=1).values
    near = (top2[:, 0] - top2[:, 1]) <= 2 * bound
    assert near.double().mean().item() <= 0.005
    g = _rounded(torch.randn(M, 8 * c), dt)
    out_g, idx_g, dx_g = run_canonize(_pack(x8), mod.reference.detach(), g, c, dt, "packed")
    assert torch.equal(idx_g[~near], idx0[~near])
    assert ((dots.max(1).values - dots.gather(1, idx_g.unsqueeze(1)).squeeze(1)) <= 2 * bound).all()
    mats = _mats()
    assert _same(out_g, torch.einsum("tij,tjc->tic", mats[idx_g], x8).flatten(1))            # a signed copy: exact
    assert _same(dx_g, _pack(torch.einsum("tij,tic->tjc", mats[idx_g], g.view(M, 8, c))))


# ------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_rows_do_not_depend_on_batch_mates_or_position(dtn):
    dt, c, R, M = DT[dtn], 24, 40, 150
    torch.manual_seed(3)
    x = torch.randn(M, 8 * c, device=DEV).to(dt)
    ref = torch.randn(R, c, 8, device=DEV)
    gq = torch.randn(M, R, device=DEV).to(dt)
    refv = torch.randn(8 * c, device=DEV)

    def run(xx, gg):
        planes = ops.max_filter_prep(ref, dt)
        out, idx = ops.max_filter_fwd(xx, planes, c, dt)
        co, ci = ops.canonize_fwd(xx, refv, c, dt)
        return out, idx, ops.max_filter_bwd_x(gg, idx, planes, c), co, ci, ops.max_filter_bwd_ref(gg, idx, xx, c)

    a, b = run(x, gq), run(x, gq)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two calls differ"
    perm = torch.randperm(M, device=DEV)[:77]
    s = run(x[perm].contiguous(), gq[perm].contiguous())
    for k in range(5):
        assert torch.equal(s[k], a[k][perm]), k


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
def test_max_filter_is_bitwise_invariant_on_exact_products(dtn):
    dt, c, R, M = DT[dtn], 24, 40, 70
    gen = torch.Generator().manual_seed(11)
    x8, ref = _ints((M, 8, c), -3, 3, gen), _ints((R, c, 8), -2, 2, gen)
    planes = ops.max_filter_prep(ref.float().to(DEV), dt)
    base = ops.max_filter_fwd(_pack(x8).to(dt).to(DEV), planes, c, dt)[0]
    for g in range(8):
        moved = ops.max_filter_fwd(_pack(_act(g, x8)).to(dt).to(DEV), planes, c, dt)[0]
        assert torch.equal(moved, base), g


# ------------------------------------------------------------------------------------------ memory
def _tuple5(xp, c):
    return OF.Octic(xp, c)


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("which", ["max_filtering", "canonization"])
def test_peak_memory_stays_below_one_expanded_tensor(which, dtn, monkeypatch):
    """Peak allocation over forward + backward minus what must exist (input, output, their gradients' storage, saved x and idx)
    stays below ONE [M, 8, R] (MaxFiltering) / [M, 8, 8c] (Canonization) tensor of the compute dtype; the stock composition
    exceeds it."""
    dt, M, c, R = DT[dtn], 2056, 40, 640
    es = 2 if dt == torch.bfloat16 else 4
    torch.manual_seed(0)
    mod = (INV.MaxFilteringInvariant(8 * c, num_references=R) if which == "max_filtering" else INV.CanonizationInvariant(8 * c)).to(DEV)
    width = R if which == "max_filtering" else 8 * c
    expanded = M * 8 * width * es
    x = torch.randn(8, M // 8, 8 * c, device=DEV).requires_grad_()             # f32 stream; bf16 is the autocast compute dtype
    gout = torch.randn(8, M // 8, width, device=DEV, dtype=dt)

    def extra(hip):
        monkeypatch.setattr(INV, "ORBIT_HIP", hip)
        x.grad = None
        mod.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
            y = mod(_tuple5(x, c))
        assert y.dtype == dt
        y.backward(gout)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        # output, x.grad (f32), the saved x (compute dtype; MaxFiltering only) and idx, and the parameter gradient
        saved = M * R + x.numel() * es if which == "max_filtering" else M
        must = y.numel() * es + x.numel() * 4 + saved + sum(p.grad.numel() * 4 for p in mod.parameters() if p.grad is not None)
        del y
        return peak - must

    hip, stock = extra(True), extra(False)
    print(f"{which} {dtn}: engine extra {hip / 2 ** 20:.1f} MiB, stock extra {stock / 2 ** 20:.1f} MiB, one expanded tensor {expanded / 2 ** 20:.1f} MiB")
    assert hip < expanded
    assert stock > expanded


# ------------------------------------------------------------------------------------------ modules and models
def _mf_bounds(x8, ref, c, R):
    """float64 products [M, 8, R], the per-product bound (8c + 8) 2^-24 max_g sum |A_g| |x| |ref| and the near-tie mask."""
    prod, idx0, _, _ = oracle_max_filter(x8, ref)
    amats = _mats().abs()
    mag = torch.einsum("tic,gdic->tgd", x8.abs(), torch.einsum("gij,dcj->gdic", amats, ref.abs())).max(dim=1).values
    bound = (8 * c + 8) * 2.0 ** -24 * mag
    top2 = prod.topk(2, dim=1).values
    return prod, idx0, bound, (top2[:, 0] - top2[:, 1]) <= 2 * bound


@pytest.mark.parametrize("global_avg", [False, True])
def test_max_filtering_module_both_arms_against_float64(global_avg, monkeypatch):
    """Engine arm and stock arm of the module, each against the float64 oracle within the derived per-element bounds (f32: no
    rounding of stored results).  The cotangent is zero on near ties, so no gradient depends on a choice there; on every other
    pair both arms have the oracle's winner, as their products are within the bound.  The stock arm sums the same terms (its
    expanded references are signed copies; zeros of the scattered cotangent add exactly), so the same bounds cover it."""
    c, R = 16, 72
    torch.manual_seed(1)
    mod = INV.MaxFilteringInvariant(8 * c, num_references=R, global_avg=global_avg).to(DEV)
    shape = (6, 8 * c) if global_avg else (3, 43, 8 * c)
    xp = torch.randn(*shape, device=DEV)
    M = xp.numel() // (8 * c)
    x8, ref = _unpack(xp.cpu().double().view(M, 8 * c), c), mod.references.detach().cpu().double()
    prod, idx0, bound, near = _mf_bounds(x8, ref, c, R)
    assert near.double().mean().item() <= 0.005
    gy = torch.where(near, 0.0, torch.cos(torch.arange(M * R, dtype=torch.float64)).view(M, R)).float().double()
    _, _, dx, dref = oracle_max_filter(x8, ref, gy, idx=idx0)
    amats, eps = _mats().abs(), 2.0 ** -24
    Wabs = torch.zeros_like(prod).scatter_(1, idx0.unsqueeze(1), gy.abs().unsqueeze(1))
    dx_tol = _pack((2 * R + 2) * eps * torch.einsum("tgd,gdic->tic", Wabs, torch.einsum("gij,dcj->gdic", amats, ref.abs())))
    slabs = ops.max_filter_bwd_ref_plan(M, R, c)[0]
    dref_tol = (2 * M + 2 + slabs) * eps * torch.einsum("tgd,gij,tic->dcj", Wabs, amats, x8.abs())
    for hip in (True, False):
        monkeypatch.setattr(INV, "ORBIT_HIP", hip)
        x = xp.clone().requires_grad_()
        mod.zero_grad(set_to_none=True)
        y = mod(_tuple5(x, c) if hip else ops.split_packed(x, c))
        assert y.shape == (*shape[:-1], R) and y.dtype == torch.float32
        y.backward(gy.float().to(DEV).view_as(y))
        arm = "engine" if hip else "stock"
        for name, got, want, tol in (("out", y.detach().view(M, R), prod.max(dim=1).values, bound),
                                     ("dx", x.grad.view(M, 8 * c), _pack(dx), dx_tol),
                                     ("dref", mod.references.grad, dref, dref_tol)):
            err = (got.cpu().double() - want).abs()
            print(f"{arm} {name}: max err / bound {(err / tol.clamp_min(1e-300)).max().item():.3f}")
            assert (err <= tol).all(), (arm, name)


@pytest.mark.parametrize("global_avg", [False, True])
def test_canonization_module_both_arms_against_float64(global_avg, monkeypatch):
    """Both arms pick the oracle's element on every row that is no near tie (bound as for MaxFiltering with one reference), and
    there out is the signed copy and dx its inverse, exactly (f32)."""
    c = 16
    torch.manual_seed(1)
    mod = INV.CanonizationInvariant(8 * c, global_avg=global_avg).to(DEV)
    shape = (6, 8 * c) if global_avg else (3, 43, 8 * c)
    xp = torch.randn(*shape, device=DEV)
    M = xp.numel() // (8 * c)
    x8, refv = _unpack(xp.cpu().double().view(M, 8 * c), c), mod.reference.detach().cpu().double()
    dots, idx0, out0 = oracle_canonize(x8, refv, c)
    mag = torch.einsum("tgic,ic->tg", torch.einsum("gij,tjc->tgic", _mats().abs(), x8.abs()), refv.abs().view(8, c)).max(1).values
    top2 = dots.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2 * (8 * c + 8) * 2.0 ** -24 * mag
    assert sure.double().mean().item() >= 0.995
    gy = torch.cos(torch.arange(M * 8 * c, dtype=torch.float64)).view(M, 8 * c).float().double()
    dx0 = _pack(torch.einsum("tij,tic->tjc", _mats()[idx0], gy.view(M, 8, c)))
    for hip in (True, False):
        monkeypatch.setattr(INV, "ORBIT_HIP", hip)
        x = xp.clone().requires_grad_()
        y = mod(_tuple5(x, c) if hip else ops.split_packed(x, c))
        assert y.shape == shape and y.dtype == torch.float32
        y.backward(gy.float().to(DEV).view_as(y))
        assert _same(y.detach().view(M, 8 * c).cpu()[sure], out0[sure]), hip
        assert _same(x.grad.view(M, 8 * c).cpu()[sure], dx0[sure]), hip
        assert mod.reference.grad is None


def test_frozen_references_skip_their_gradient():
    c = 8
    mod = INV.MaxFilteringInvariant(8 * c, num_references=24, learnable_references=False).to(DEV)
    x = torch.randn(2, 5, 8 * c, device=DEV, requires_grad=True)
    mod(_tuple5(x, c)).sum().backward()
    assert x.grad is not None and mod.references.grad is None


def _inv_model(seed=0):
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(seed)
    return OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=2, num_heads=2,
                                  mlp_ratio=4.0, drop_path_rate=0.0, invariant=True, invariantization="max_filtering").cuda()


def test_max_filtering_model_trains_eager_and_captured_bitwise():
    from octic_vits_amd.train import Trainer, synthetic_batch
    ma, mb = _inv_model(), _inv_model()
    assert isinstance(ma.invariantization, INV.MaxFilteringInvariant) and ma.invariant_proj.in_features == 256
    ta, tb = Trainer(ma, lr=1e-3), Trainer(mb, lr=1e-3)
    batches = [synthetic_batch(8, 10, "cuda", seed=s, img_size=32) for s in range(3)]
    gs = tb.capture(*batches[0], warmup=2)
    for _ in range(2):
        ta.step(*batches[0])
    r0 = ma.invariantization.references.detach().clone()
    la = [float(ta.step(x, y).detach()) for x, y in batches[1:]]
    lb = [float(gs.replay(x, y)) for x, y in batches[1:]]
    assert la == lb and all(v == v for v in la)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa, pb), n
    assert not torch.equal(r0, ma.invariantization.references)           # the references are a parameter of the fused optimizer


def test_max_filtering_model_first_backward_against_float64():
    """One Trainer.step of the 2-block "max_filtering" model (bf16 autocast), checked at its first backward against float64
    through the model's own wiring: hooks take the block output the hand-off receives, the map's output, the projection's
    output and the cotangents that arrive at each; parameter hooks take the gradients of references, invariant_proj.weight and
    invariant_proj.bias.  float64 replicas of the map and of the projection run on those operands rounded as the step rounds
    them (bf16), and every tensor is compared within its f32 summation bound plus half a bf16 ulp where it is stored in bf16."""
    from octic_vits_amd.train import Trainer, synthetic_batch
    bf = torch.bfloat16
    net = _inv_model(seed=3)
    inv, proj = net.invariantization, net.invariant_proj
    cap, grads = {}, {}

    def pre(mod, args, kwargs):
        xs = args[0]
        assert isinstance(xs, OF.Octic)
        cap["x"], cap["c"], cap["out_dtype"] = xs.packed.detach().clone(), xs.c, kwargs.get("_out_dtype")
        xs.packed.register_hook(lambda g: cap.__setitem__("dx", g.detach().clone()))

    def post(mod, args, kwargs, out):
        cap["y"] = out.detach().clone()
        out.register_hook(lambda g: cap.__setitem__("gy", g.detach().clone()))

    def proj_post(mod, args, out):
        cap["proj_in"], cap["z"] = args[0].detach().clone(), out.detach().clone()
        out.register_hook(lambda g: cap.__setitem__("gz", g.detach().clone()))

    hs = [inv.register_forward_pre_hook(pre, with_kwargs=True), inv.register_forward_hook(post, with_kwargs=True),
          proj.register_forward_hook(proj_post)]
    for n, p in (("references", inv.references), ("weight", proj.weight), ("bias", proj.bias)):
        hs.append(p.register_hook(lambda g, n=n: grads.__setitem__(n, g.detach().clone())))
    r0, w0, b0 = (t.detach().clone() for t in (inv.references, proj.weight, proj.bias))
    tr = Trainer(net, lr=1e-3)
    assert any(p is inv.references for p in tr.optimizer.params), "references must be a parameter of the fused optimizer"
    loss = float(tr.step(*synthetic_batch(8, 10, "cuda", seed=1, img_size=32)))
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    assert loss == loss and not torch.equal(r0, inv.references)
    c, R, eps = cap["c"], r0.shape[0], 2.0 ** -24
    x, y = cap["x"], cap["y"]
    Bq, Tq = x.shape[:2]
    M, D = Bq * Tq, w0.shape[0]
    assert c == 16 and x.dtype == torch.float32 and cap["out_dtype"] == bf and y.dtype == bf and y.shape == (Bq, Tq, R)
    assert torch.equal(cap["proj_in"], y) and cap["gy"].dtype == bf and cap["dx"].dtype == torch.float32
    assert grads["references"].dtype == torch.float32 and grads["references"].shape == r0.shape
    # the map, forward: the step ran this kernel on these rows (same bits), and that is the float64 result within the bound
    out_g, idx_g = ops.max_filter_fwd(x.view(M, 8 * c).to(bf), ops.max_filter_prep(r0, bf), c, bf)
    assert torch.equal(out_g.view_as(y), y)
    x8, ref = _unpack(x.view(M, 8 * c).to(bf).cpu().double(), c), r0.to(bf).cpu().double()
    prod, idx0, bound, near = _mf_bounds(x8, ref, c, R)
    idx_g = idx_g.cpu().long()
    # No cap on the share of near ties here: these are a model's activations, not seeded noise.  At initialisation the
    # class-token row of every image is a near tie against every reference (its non-invariant components are almost zero:
    # only the A1 class-token parameter is non-zero), 1 / T of the rows; the candidate rule below covers them.
    print(f"model near ties: {100 * near.double().mean().item():.3f} % of {M * R} pairs")
    assert torch.equal(idx_g[~near], idx0[~near])
    best = prod.max(dim=1).values
    assert ((best - prod.gather(1, idx_g.unsqueeze(1)).squeeze(1)) <= 2 * bound).all()
    y64 = y.view(M, R).cpu().double()
    assert ((y64 - best).abs() <= bound + _half_ulp(best, bf)).all(), "map output"
    # the map, backward, with the winners the step used and the cotangent that reached it
    gy = cap["gy"].view(M, R).cpu().double()
    _, _, dx, dref = oracle_max_filter(x8, ref, gy, idx=idx_g)
    amats = _mats().abs()
    Wabs = torch.zeros_like(prod).scatter_(1, idx_g.unsqueeze(1), gy.abs().unsqueeze(1))
    dx_tol = _pack((2 * R + 2) * eps * torch.einsum("tgd,gdic->tic", Wabs, torch.einsum("gij,dcj->gdic", amats, ref.abs()))) + _half_ulp(_pack(dx), bf)
    dx_err = (cap["dx"].view(M, 8 * c).cpu().double() - _pack(dx)).abs()
    print(f"model dx: max err / bound {(dx_err / dx_tol.clamp_min(1e-300)).max().item():.3f}")
    assert (dx_err <= dx_tol).all(), "cotangent at the block output"
    slabs = ops.max_filter_bwd_ref_plan(M, R, c)[0]
    dref_tol = (2 * M + 2 + slabs) * eps * torch.einsum("tgd,gij,tic->dcj", Wabs, amats, x8.abs())
    dref_err = (grads["references"].cpu().double() - dref).abs()
    print(f"model dref: max err / bound {(dref_err / dref_tol.clamp_min(1e-300)).max().item():.3f}")
    assert (dref_err <= dref_tol).all(), "references.grad"
    # invariant_proj under bf16 autocast: bf16 operands (input, weight, bias), f32 sums, results stored in bf16
    W, b = w0.to(bf).cpu().double(), b0.to(bf).cpu().double()
    gz = cap["gz"].view(M, D).cpu().double()
    assert cap["z"].dtype == bf and cap["gz"].dtype == bf

    def check(name, got, want, mag, n):
        tol = (n + 2) * eps * mag + _half_ulp(want, bf)
        err = (got.cpu().double() - want).abs()
        print(f"model {name}: max err / bound {(err / tol.clamp_min(1e-300)).max().item():.3f}")
        assert (err <= tol).all(), name

    check("proj output", cap["z"].view(M, D), y64 @ W.t() + b, y64.abs() @ W.abs().t() + b.abs(), R + 1)
    check("cotangent at the map output", cap["gy"].view(M, R), gz @ W, gz.abs() @ W.abs(), D)
    check("invariant_proj.weight.grad", grads["weight"], gz.t() @ y64, gz.abs().t() @ y64.abs(), M)
    check("invariant_proj.bias.grad", grads["bias"], gz.sum(0), gz.abs().sum(0), M)


def _dino_model(name):
    from octic_vits_amd import d8_layers, dinov2_models, vit
    torch.manual_seed(0)
    return dinov2_models.OcticDinoVisionTransformer(
        img_size=32, patch_size=4, embed_dim=128, depth=4, num_heads=4, invariant=True, invariantization=name,
        octic_block_layers=lambda **kw: d8_layers.NestedTensorBlockD8(init_values=0.1, **{k: v for k, v in kw.items() if k != "init_values"}),
        standard_block_layers=lambda **kw: vit.NestedTensorBlock(attn_class=vit.MemEffAttention, init_values=0.1,
                                                                 **{k: v for k, v in kw.items() if k != "init_values"})).cuda()


@pytest.mark.parametrize("name", ["linear", "polynomial", "third_order", "canonization", "max_filtering"])
def test_every_map_runs_at_the_three_call_sites(name):
    """model.py, dinov2_models.py and train.py's slices pass an Octic and `_out_dtype`; every map must take both."""
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.train import SegmentedModel
    x = torch.randn(4, 3, 32, 32, device=DEV)
    torch.manual_seed(0)
    net = OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=2, num_heads=2,
                                 invariant=True, invariantization=name).cuda()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = net(x)
    y.float().square().mean().backward()
    assert torch.isfinite(y).all() and torch.isfinite(net.invariant_proj.weight.grad).all()
    net.zero_grad(set_to_none=True)
    ys = SegmentedModel(net, 2)(x)
    ys.float().square().mean().backward()
    assert ys.shape == y.shape and torch.isfinite(ys).all() and torch.isfinite(net.invariant_proj.weight.grad).all()
    dino = _dino_model(name)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = dino.forward_features(x)["x_norm_clstoken"]
    out.float().square().mean().backward()
    assert torch.isfinite(out).all() and torch.isfinite(dino.invariant_proj.weight.grad).all()


def test_workspace_too_small_and_fp16_autocast_predicate():
    """The workspace check of the reference gradient on real, fully sized buffers (only the stated size is short); and the
    predicate under fp16 autocast: float32 inputs go to the kernels (in float32), bf16 inputs stay on the stock arm."""
    M, c, R = 70, 8, 24
    g = torch.zeros(M, R, device=DEV)
    idx = torch.zeros(M, R, dtype=torch.uint8, device=DEV)
    x = torch.zeros(M, 8 * c, device=DEV)
    need = int(lib().octic_max_filter_bwd_ref_workspace_bytes(M, R, c))
    ws, dref = torch.zeros(need, dtype=torch.uint8, device=DEV), torch.zeros(R, c, 8, device=DEV)
    xv = ops.pview(x, c)
    assert lib().octic_max_filter_bwd_ref(_p(g), _p(idx), ctypes.byref(xv), _p(dref), _p(ws), need - 1, M, R, c, _lib.F32, _stream()) == -5
    ref = torch.zeros(R, c, 8, device=DEV)
    with torch.autocast("cuda", dtype=torch.float16):
        assert INV.orbit_hip_ok(OF.Octic(x, c), ref)
        assert not INV.orbit_hip_ok(OF.Octic(x.bfloat16(), c), ref)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert INV.orbit_hip_ok(OF.Octic(x.bfloat16(), c), ref) and INV.orbit_hip_ok(OF.Octic(x, c), ref)
