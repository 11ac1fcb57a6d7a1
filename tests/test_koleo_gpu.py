"""KoLeo kernels (csrc/koleo.hip: ops.koleo_fwd / koleo_bwd, functional.KoLeoFn, ssl.KoLeoLoss) on the GPU.

Yardsticks: exact integer arithmetic on planted rows for the neighbour search and its total order; the reference's own numbers
(tests/golden/ssl_pieces.npz); float64 autograd of the reference formula with the kernel's neighbours forced; the f32 eager
composition (``FUSED_LOSS_ROWS = False``) on the same device and inputs.

ERROR BOUND of every float comparison (``_bound``): the larger of (a) twice the error of the f32 eager arm against the same
float64 values - twice because the two arms round sums of the same length in different orders - and (b) D * 2^-24 relative to
the largest magnitude of the compared tensor, the floor for inputs where the eager arm happens to be exact.  A bf16 gradient
gets one bf16 ulp of the element on top (it is rounded once).  The eager arm of these comparisons has its neighbours forced to
the kernel's as well, so its error is rounding alone and a different choice on a near tie cannot widen the bound.
NEIGHBOURS on Gaussian rows are accepted when the float64 dot of the chosen row is within tau = 2 (D + 4) 2^-24 of the float64
maximum: the worst-case rounding of two unit-norm length-D f32 dots."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-8
N_MAX = 256
DTYPES = [torch.float32, torch.bfloat16]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rows(x, groups, nn, dtype):
    """The reference formula (koleo_loss.py:25-48 without the mean) in `dtype` with the neighbours forced to the group-local
    indices nn: (terms [rows], the leaf they hang on)."""
    leaf = x.detach().to(dtype).requires_grad_(True)
    n = x.shape[0] // groups
    idx = nn.long() + (torch.arange(x.shape[0], device=x.device) // n) * n
    xh = F.normalize(leaf, eps=EPS, p=2, dim=-1)
    d = torch.nn.PairwiseDistance(2, eps=1e-8)(xh, xh[idx])
    return -torch.log(d + EPS), leaf


def _bf16_ulp(v):
    v = v.abs().double().clamp(min=2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(v)) - 7)


def _bound(eager, ref, D):
    """max |error| allowed against ref (float64): see the module docstring."""
    return max(2.0 * float((eager.double() - ref).abs().max()), D * 2.0 ** -24 * float(ref.abs().max()))


def _fused(x, groups, w):
    """Kernel arm: (term, nn, dx) for the loss sum(term * w)."""
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ops
    leaf = x.detach().clone().requires_grad_(True)
    assert OF.koleo_rows_ok(leaf, groups)
    term = OF.KoLeoFn.apply(leaf, groups, EPS)
    (term * w).sum().backward()
    nn = ops.koleo_fwd(x, groups, EPS)[1]
    return term.detach(), nn, leaf.grad


def _check_against_float64(x, groups, seed, label=""):
    """term and dx of the kernels against float64 autograd with the kernel's nn forced, inside the bound the eager arm sets."""
    D = x.shape[1]
    w = torch.rand(x.shape[0], generator=_gen(seed), device="cuda") + 0.5
    term, nn, dx = _fused(x, groups, w)
    assert dx.dtype == x.dtype and dx.shape == x.shape
    t64, l64 = _rows(x, groups, nn, torch.float64)
    (t64 * w.double()).sum().backward()
    t32, l32 = _rows(x, groups, nn, torch.float32)
    (t32 * w).sum().backward()
    bt, bg = _bound(t32.detach(), t64.detach(), D), _bound(l32.grad, l64.grad, D)
    et = float((term.double() - t64.detach()).abs().max())
    extra = _bf16_ulp(l64.grad) if x.dtype == torch.bfloat16 else 0.0
    over = ((dx.double() - l64.grad).abs() - extra - bg).max()
    eg = float((dx.double() - l64.grad).abs().max())
    print(f"koleo {label} {str(x.dtype)[6:]} rows {x.shape[0]} D {D} G {groups}: term err kernels {et:.3e} eager "
          f"{float((t32.detach().double() - t64.detach()).abs().max()):.3e} bound {bt:.3e} | dx err kernels {eg:.3e} eager "
          f"{float((l32.grad.double() - l64.grad).abs().max()):.3e} bound {bg:.3e} (max |dx| {float(l64.grad.abs().max()):.3e})")
    assert torch.isfinite(term).all() and torch.isfinite(dx.float()).all()
    assert et <= bt, (et, bt)
    assert float(over) <= 0.0, (eg, bg)
    return term, nn, dx


# ------------------------------------------------------------------------------------------------ exact neighbours
def _planted(n, D, G, seed):
    """[G * n, D] int8 rows with exactly four entries of +-1: norm 2, xh = +-0.5, every dot a multiple of 0.25 and exact in f32
    and bf16 under any summation order.  Planted: the last row of a group is the twin of its row 0 (the twin must be found,
    never the row itself); row 1 is row 0 with one sign flipped (equal dots with both twins: the lowest index wins); row 2 is a
    row whose unique best match is row 1 where the rest allows it; group 1's row 0 is a copy of group 0's row 1 (a perfect match
    in ANOTHER group that must not be seen)."""
    rng = np.random.RandomState(seed)
    x = np.zeros((G * n, D), dtype=np.int8)
    for r in range(G * n):
        pos = rng.choice(D, 4, replace=False)
        x[r, pos] = rng.choice([-1, 1], 4)
    for g in range(G):
        b = g * n
        if n >= 3:
            x[b + 1] = x[b]
            x[b + 1, np.flatnonzero(x[b])[0]] *= -1
        if n >= 4:
            x[b + 2] = 0
            nz = np.flatnonzero(x[b + 1])
            x[b + 2, nz[:3]] = x[b + 1, nz[:3]]
            free = [k for k in range(D) if x[b, k] == 0 and x[b + 1, k] == 0]
            x[b + 2, free[g % len(free)]] = 1
        x[b + n - 1] = x[b]
    if G > 1 and n >= 3:
        x[n] = x[1]
        x[2 * n - 1] = x[n]
    return x


def _expected_nn(x, n, G):
    out = []
    for g in range(G):
        xs = x[g * n:(g + 1) * n].astype(np.int64)
        m = xs @ xs.T
        np.fill_diagonal(m, -100)
        out.append(np.argmax(m, axis=1))               # first occurrence: the lowest index on equal dots
    return np.concatenate(out)


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("D", [8, 72, 1280])
@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 129, 256])
def test_planted_rows_give_exact_neighbours(n, D, G):
    from octic_vits_amd import ops
    x = _planted(n, D, G, seed=1000 * n + D + G)
    want = _expected_nn(x, n, G)
    full = x.astype(np.int64) @ x.astype(np.int64).T
    np.fill_diagonal(full, -100)
    own = np.array([full[r, (r // n) * n:(r // n + 1) * n].max() for r in range(G * n)])
    # the construction holds what it promises (checked on the integers, before any kernel runs)
    assert want[0] != 0 and full[0, want[0]] == 4                                   # a twin, not the row itself
    if n >= 3:
        rows = np.arange(G * n)
        grp = full[rows[:, None], ((rows // n) * n)[:, None] + np.arange(n)[None, :]]
        ties = (grp == own[:, None]).sum(1)
        assert (ties >= 2).any() and (ties == 1).any()                              # a tie at the maximum and a unique best
        if n == 3:
            assert want[1] == 0                                                     # both twins are equally good: the lower
    if G > 1 and n >= 3:
        assert (full.max(1) > own).any()                                            # a better match in another group
    for dt in DTYPES:
        t = torch.from_numpy(x.astype(np.float32)).cuda().to(dt)
        term, nn, inv, dist = ops.koleo_fwd(t, G, EPS)
        assert nn.dtype == torch.int32
        assert np.array_equal(nn.cpu().numpy(), want), (dt, np.flatnonzero(nn.cpu().numpy() != want)[:8])
        assert torch.equal(inv, torch.full_like(inv, 0.5))
        assert torch.isfinite(term).all()


# ------------------------------------------------------------------------------------------------ the reference's numbers
def test_reference_golden_case():
    from octic_vits_amd import ssl as S
    want = np.load(os.path.join(GOLD, "ssl_pieces.npz"))
    D = want["koleo.gx"].shape[1]
    x0 = cases.randn("ssl.koleo.x", 10, D).cuda()

    def run(fused):
        S.FUSED_LOSS_ROWS = fused
        try:
            x = x0.clone().requires_grad_(True)
            loss = S.KoLeoLoss()(x)
            loss.backward()
            return loss.detach().double().cpu().numpy().reshape(1), x.grad.double().cpu().numpy()
        finally:
            S.FUSED_LOSS_ROWS = True

    (lk, gk), (le, ge) = run(True), run(False)
    wl, wg = want["koleo.loss"].astype(np.float64), want["koleo.gx"].astype(np.float64)
    bl = max(2 * np.abs(le - wl).max(), D * 2.0 ** -24 * np.abs(wl).max())
    bg = max(2 * np.abs(ge - wg).max(), D * 2.0 ** -24 * np.abs(wg).max())
    print(f"koleo golden: loss err kernels {np.abs(lk - wl).max():.3e} eager {np.abs(le - wl).max():.3e} bound {bl:.3e} | gx err "
          f"kernels {np.abs(gk - wg).max():.3e} eager {np.abs(ge - wg).max():.3e} bound {bg:.3e}")
    assert np.abs(lk - wl).max() <= bl and np.abs(gk - wg).max() <= bg
    from octic_vits_amd import ops
    xh = F.normalize(x0.double().cpu(), eps=EPS, dim=-1)
    dots = xh @ xh.t()
    dots.fill_diagonal_(-2)
    assert torch.equal(ops.koleo_fwd(x0, 1, EPS)[1].cpu().long(), dots.argmax(1))


# ------------------------------------------------------------------------------------------------ float64 oracle
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("D", [64, 384, 1536])
@pytest.mark.parametrize("n", [5, 32, 65])
def test_gaussian_rows_against_float64(n, D, G, dtype):
    x = torch.randn(G * n, D, generator=_gen(7 * n + D + G), device="cuda").to(dtype)
    term, nn, dx = _check_against_float64(x, G, seed=3, label="gaussian")
    xh = F.normalize(x.double(), eps=EPS, dim=-1).view(G, n, D)
    dots = xh @ xh.transpose(1, 2)
    dots.diagonal(dim1=1, dim2=2).fill_(-2)
    chosen = dots.gather(2, nn.view(G, n, 1).long()).squeeze(2)
    tau = 2 * (D + 4) * 2.0 ** -24
    assert ((nn.view(G, n) >= 0) & (nn.view(G, n) < n)).all()
    assert (nn.view(G, n) != torch.arange(n, device="cuda")).all()
    assert (chosen >= dots.max(2)[0] - tau).all()


# ------------------------------------------------------------------------------------------------ invariances, bitwise
def _all(x, groups, w):
    from octic_vits_amd import ops
    term, nn, inv, dist = ops.koleo_fwd(x, groups, EPS)
    return term, nn, inv, dist, ops.koleo_bwd(x, groups, w, nn, inv, dist, EPS)


@pytest.mark.parametrize("dtype", DTYPES)
def test_results_do_not_depend_on_groups_position_strides_or_the_rest_of_the_batch(dtype):
    n, D, G = 37, 136, 3
    x = torch.randn(G * n, D, generator=_gen(21), device="cuda").to(dtype)
    w = torch.rand(G * n, generator=_gen(22), device="cuda")
    base = _all(x, G, w)
    for a, b in zip(base, _all(x, G, w)):                                 # two calls
        assert torch.equal(a, b)
    for g in range(G):                                                    # a group alone
        alone = _all(x[g * n:(g + 1) * n].clone(), 1, w[g * n:(g + 1) * n].clone())
        for a, b in zip(base, alone):
            assert torch.equal(a[g * n:(g + 1) * n], b), g
    wide = torch.full((G * n, D + 8), 7.0, device="cuda", dtype=dtype)    # a row-strided view
    wide[:, :D] = x
    view = wide[:, :D]
    assert view.stride(0) == D + 8 and not view.is_contiguous()
    from octic_vits_amd import functional as OF
    assert OF.koleo_rows_ok(view, G)
    for a, b in zip(base, _all(view, G, w)):
        assert torch.equal(a, b)
    other = x.clone()                                                     # other groups' values change
    other[:n] = torch.randn(n, D, generator=_gen(23), device="cuda").to(dtype)
    other[2 * n:] = 0
    for a, b in zip(base, _all(other, G, w)):
        assert torch.equal(a[n:2 * n], b[n:2 * n])
    leaf = view.detach().requires_grad_(True)                             # the autograd function on the strided view
    (OF.KoLeoFn.apply(leaf, G, EPS) * w).sum().backward()
    assert torch.equal(leaf.grad, base[4])


# ------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize("n", [2, 5])
def test_zero_row(n):
    x = torch.randn(n, 64, generator=_gen(31), device="cuda")
    x[1] = 0
    term, nn, dx = _check_against_float64(x, 1, seed=4, label="zero row")
    assert int(nn[1]) == 0                                                # every dot of the zero row is 0: the lowest other index


@pytest.mark.parametrize("scale", [1e-3, 1e3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_small_and_large_norm(scale, dtype):
    x = torch.randn(9, 72, generator=_gen(33), device="cuda")
    x = (x / x.norm(dim=1, keepdim=True) * scale).to(dtype)
    _check_against_float64(x, 1, seed=5, label=f"norm {scale:g}")


@pytest.mark.parametrize("row", [0, 3])
def test_bf16_extremes_are_finite_where_the_eager_arm_is(row):
    """A row of +-bf16 max: its squared norm overflows f32, so F.normalize makes it the zero row in both arms.  float64 is no
    yardstick here (nothing overflows there), the eager arm is: the loss within D 2^-24 of it (one such row per case: all its
    dots are 0, the arms may choose different neighbours for it, and every choice among unit rows moves the loss by ~1e-8)."""
    from octic_vits_amd import ssl as S
    big = float(torch.finfo(torch.bfloat16).max)
    x0 = torch.randn(6, 64, generator=_gen(35), device="cuda")
    x0[row] = torch.where(x0[row] > 0, big, -big)
    x0 = x0.to(torch.bfloat16)

    def run(fused):
        S.FUSED_LOSS_ROWS = fused
        try:
            x = x0.clone().requires_grad_(True)
            loss = S.KoLeoLoss()(x)
            loss.backward()
            return loss.detach(), x.grad
        finally:
            S.FUSED_LOSS_ROWS = True

    (le, ge), (lk, gk) = run(False), run(True)
    print(f"koleo bf16 extremes: loss kernels {float(lk):.7g} eager {float(le):.7g}")
    if torch.isfinite(le) and torch.isfinite(ge.float()).all():
        assert torch.isfinite(lk) and torch.isfinite(gk.float()).all()
        assert abs(float(lk) - float(le)) <= 64 * 2.0 ** -24 * max(1.0, abs(float(le)))


def test_zero_cotangent_gives_zero_gradient():
    from octic_vits_amd import ops
    x = torch.randn(2 * 17, 40, generator=_gen(37), device="cuda").to(torch.bfloat16)
    term, nn, inv, dist = ops.koleo_fwd(x, 2, EPS)
    dx = ops.koleo_bwd(x, 2, torch.zeros_like(term), nn, inv, dist, EPS)
    assert torch.equal(dx.float(), torch.zeros(34, 40, device="cuda"))


# ------------------------------------------------------------------------------------------------ routing
def _module_both_ways(x0):
    from octic_vits_amd import ssl as S
    out = []
    for fused in (True, False):
        S.FUSED_LOSS_ROWS = fused
        try:
            x = x0.detach().clone().requires_grad_(True) if x0.is_contiguous() else x0.detach().requires_grad_(True)
            loss = S.KoLeoLoss()(x)
            loss.backward()
            out.append((loss.detach(), x.grad))
        finally:
            S.FUSED_LOSS_ROWS = True
    return out


@pytest.mark.parametrize("case", ["n=1", "n=n_max+1", "D=12", "fp16", "transposed"])
def test_shapes_outside_the_range_take_the_eager_path(case, monkeypatch):
    """Outside octic_koleo_ok, in fp16 and on a transposed view the module runs today's composition: no kernel call, and the
    numbers of the FUSED_LOSS_ROWS = False arm bitwise (the loss everywhere; the gradient where index_select's atomic scatter
    has a defined order, i.e. at most two rows choosing the same neighbour - at n = n_max + 1 it is compared to 1e-6 of its
    largest magnitude instead)."""
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ops
    g = _gen(41)
    x = {"n=1": lambda: torch.randn(1, 64, generator=g, device="cuda"),
         "n=n_max+1": lambda: torch.randn(N_MAX + 1, 64, generator=g, device="cuda"),
         "D=12": lambda: torch.randn(3, 12, generator=g, device="cuda"),
         "fp16": lambda: torch.randn(3, 64, generator=g, device="cuda").half(),
         "transposed": lambda: torch.randn(64, 3, generator=g, device="cuda").t()}[case]()
    assert not OF.koleo_rows_ok(x, 1)

    def refuse(*a, **k):
        raise AssertionError("the KoLeo kernels were called")
    monkeypatch.setattr(ops, "koleo_fwd", refuse)
    (la, ga), (lb, gb) = _module_both_ways(x)
    assert torch.equal(la, lb)
    if case == "n=n_max+1":
        assert float((ga - gb).abs().max()) <= 1e-6 * float(gb.abs().max())
    else:
        assert torch.equal(ga, gb)


def test_unfused_module_is_todays_composition_bitwise():
    """FUSED_LOSS_ROWS = False: the module against the composition it has always run, restated here op by op."""
    from octic_vits_amd import ssl as S
    x0 = torch.randn(3, 64, generator=_gen(43), device="cuda").to(torch.bfloat16)
    S.FUSED_LOSS_ROWS = False
    try:
        a = x0.clone().requires_grad_(True)
        la = S.KoLeoLoss()(a)
        la.backward()
    finally:
        S.FUSED_LOSS_ROWS = True
    b = x0.clone().requires_grad_(True)
    with torch.autocast(device_type="cuda", enabled=False):
        xh = F.normalize(b.float(), eps=1e-8, p=2, dim=-1)
        dots = torch.mm(xh, xh.t())
        dots.view(-1)[::4].fill_(-1)
        idx = torch.max(dots, dim=1)[1]
        lb = -torch.log(torch.nn.PairwiseDistance(2, eps=1e-8)(xh, xh[idx]) + 1e-8).mean()
    lb.backward()
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(a.grad, b.grad)


# ------------------------------------------------------------------------------------------------ in the step
def _arch(seed=0, **kw):
    from octic_vits_amd import ssl as S
    from test_ssl_gpu import DIM, KW, _product_backbone
    torch.manual_seed(seed)
    return S.SSLMetaArch(_product_backbone, DIM, koleo_loss_weight=0.1, **{**KW, **kw}).cuda().train()


def _images(B, seed):
    import random
    from octic_vits_amd import ssl as S
    random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    gc, lc = torch.randn(2 * B, 3, 32, 32, generator=g), torch.randn(2 * B, 3, 16, 16, generator=g)
    im = S.collate(gc, lc, (0.1, 0.5), 0.5, 64, S.MaskingGenerator((8, 8), max_num_patches=32))
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in im.items()}


def _step(arch, images, fused):
    from octic_vits_amd import ssl as S
    S.FUSED_LOSS_ROWS = fused
    try:
        for p in arch.student.parameters():
            p.grad = None
        out = arch.forward_backward(images, teacher_temp=0.05)
        torch.cuda.synchronize()
        return ({k: v.detach().clone() for k, v in out.items()},
                {n: p.grad.detach().clone() for n, p in arch.student.named_parameters() if p.grad is not None})
    finally:
        S.FUSED_LOSS_ROWS = True


def test_unfused_step_is_the_per_chunk_composition_bitwise(monkeypatch):
    """FUSED_LOSS_ROWS = False: SSLMetaArch.forward_backward through forward_groups against the expression it replaced,
    sum(koleo_loss(p) for p in chunk(2)) - every loss and every student gradient bitwise (two images per crop: every scatter of
    the eager backward has a defined order)."""
    from octic_vits_amd import ssl as S
    images = _images(2, 5)
    la, ga = _step(_arch(), images, False)

    class _Pair(list):
        def unbind(self, dim):
            return tuple(self)
    monkeypatch.setattr(S.KoLeoLoss, "forward_groups", lambda self, x, groups, eps=1e-8: _Pair(self(p) for p in x.chunk(groups)))
    lb, gb = _step(_arch(), images, False)
    assert set(la) == set(lb) and set(ga) == set(gb)
    for k in la:
        assert torch.equal(la[k], lb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def test_step_fused_against_unfused_f32(monkeypatch):
    """One f32 forward_backward with koleo_loss_weight = 0.1, the KoLeo kernels against the eager composition (the DINO / iBOT
    row kernels are on in both arms: only the KoLeo route differs).  The class tokens the term sees are checked first: every
    row's best neighbour leads the runner-up by more than 16 tau in float64, so both arms choose the same rows.  Bound: as in
    the module docstring, measured on those class tokens (the relative error of the eager arm's dx against float64, doubled,
    or D 2^-24), applied to koleo_loss, total and - relative to its largest magnitude - every student gradient."""
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ssl as S
    images = _images(4, 9)
    seen = []
    real = OF.koleo_rows_ok
    monkeypatch.setattr(OF, "koleo_rows_ok", lambda x, groups: (seen.append(x.detach().clone()), real(x, groups))[1])
    lf, gf = _step(_arch(), images, True)
    monkeypatch.setattr(OF, "koleo_rows_ok", lambda x, groups: False)
    lu, gu = _step(_arch(), images, True)                         # KoLeo alone off; the other loss rows stay fused
    monkeypatch.undo()
    cls = seen[0]
    G, n, D = 2, cls.shape[0] // 2, cls.shape[1]
    assert cls.dtype == torch.float32 and n == 4
    xh = F.normalize(cls.double(), eps=EPS, dim=-1).view(G, n, D)
    dots = xh @ xh.transpose(1, 2)
    dots.diagonal(dim1=1, dim2=2).fill_(-2)
    top = dots.topk(2, dim=2)[0]
    tau = 2 * (D + 4) * 2.0 ** -24
    assert float((top[..., 0] - top[..., 1]).min()) > 16 * tau
    nn = dots.argmax(2).view(-1).int()
    w = torch.full((G * n,), 1.0 / n, device="cuda")
    t64, l64 = _rows(cls, G, nn, torch.float64)
    (t64 * w.double()).sum().backward()
    t32, l32 = _rows(cls, G, nn, torch.float32)
    (t32 * w).sum().backward()
    rel = max(2 * float((l32.grad.double() - l64.grad).abs().max()) / float(l64.grad.abs().max()), D * 2.0 ** -24)
    rel_t = max(2 * float((t32.detach().double() - t64.detach()).abs().max()) / float(t64.detach().abs().max()), D * 2.0 ** -24)
    print(f"koleo step: relative bound terms {rel_t:.3e} gradients {rel:.3e}")
    assert set(lf) == set(lu)
    for k in ("koleo_loss", "total"):
        err = abs(float(lf[k]) - float(lu[k]))
        print(f"koleo step: {k} fused {float(lf[k]):.8g} unfused {float(lu[k]):.8g}")
        assert err <= rel_t * max(abs(float(lu[k])), float(t64.detach().abs().max()) * 0.1), k
    worst = 0.0
    for k in gu:
        scale = float(gu[k].abs().max())
        err = float((gf[k] - gu[k]).abs().max())
        if scale > 0:
            worst = max(worst, err / scale)
    print(f"koleo step: worst gradient difference / largest magnitude {worst:.3e}")
    for k in gu:
        assert float((gf[k] - gu[k]).abs().max()) <= rel * float(gu[k].abs().max()), k


def test_trainer_step_bf16_autocast_runs_and_is_finite():
    from octic_vits_amd import ssl as S
    arch, images = _arch(), _images(4, 9)
    out = S.SSLTrainer(arch, lr=1e-3).step(images, teacher_temp=0.05)
    assert "koleo_loss" in out and all(torch.isfinite(v).all() for v in out.values())
    assert all(torch.isfinite(p).all() for p in arch.student.parameters())
