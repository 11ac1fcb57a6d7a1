"""The octic weight gradient under the stochastic-depth mask of its branch (include/octic_hip.h: octic_linear_d8_wgrad_skip;
wgrad_ring_kernel<true>, csrc/wgrad.hip): the kernel reads only the 32-row steps that touch a kept sample and deals them evenly
over its row splits, which regroups the f32 slab sums.

bf16 on the ring route's smallest shapes, (cin, cout) = (160, 160) and (160, 320), 4 and 6 samples of 5, 33 and 257 token rows
(several samples per step; steps straddling samples; a partial last step; one split and several), with and without bias and
layer scale.

1. Exact reference: integer-valued operands whose f32 sums are exact - dw, dbias and dcs equal the unmasked launch on dY with the
   dropped rows zeroed and the float64 product, bit for bit.
2. Random operands: within the bound of a regrouped f32 sum of the float64 product (derivation at _bounds).
3. NaN in the X rows of fully dead steps changes nothing.   4. Two launches under one mask agree bit for bit.
5. Nobody kept: exact zeros, nothing read.  One kept sample of 5 rows: fewer live steps than splits.
6. f32 operands, a 96-wide shape (the tiled kernel) and a NULL mask are the plain entry's launches.
7. One training step of the model of test_linear_skip_gpu.py::test_train_step_at_257_tokens with the switch on and off under the
   same injected masks: the loss and every gradient that is not an octic LinearD8 weight, bias or layer-scale gradient are
   bitwise equal, the octic ones within the bound (float64, from the operands hooked in the step; the step runs without the
   optimizer, which rewrites the gradient buffers); the captured step equals the eager one bit for bit.
   Measured on MI355X: 22 of the 34 octic gradients move, by at most 1.2e-3 of their bound."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
KEEP = 2.0
U = 2.0 ** -23
SHAPES = [(160, 160), (160, 320)]


def _masks(B):
    out = {"all kept": [KEEP] * B, "alternating": [KEEP * (b & 1) for b in range(B)],
           "first kept": [KEEP] + [0.0] * (B - 1), "last kept": [0.0] * (B - 1) + [KEEP]}
    g = torch.Generator().manual_seed(700 + B)
    out["bernoulli"] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).tolist()
    return out


def _row_keep(mask, rps):
    return (torch.tensor(mask, device=DEV) != 0).repeat_interleave(rps)


def _groups(t, c):
    """The five reduction problems of a packed [M, 8c] tensor: A1 A2 B1 B2 as [M, c], E as [2M, 2c] (row mm = token mm >> 1)."""
    M = t.shape[0]
    return [t[:, i * c:(i + 1) * c] for i in range(4)] + [t[:, 4 * c:].reshape(2 * M, 2 * c)]


@functools.lru_cache(maxsize=None)
def _problem(cin, cout, M, integer):
    """x, dy (bf16), f32 master weights, layer scale and bias; never modified."""
    g = torch.Generator().manual_seed(cin + 7 * cout + 13 * M + integer)
    if integer:
        x = torch.randint(-2, 3, (M, 8 * cin), generator=g).to(torch.bfloat16)
        dy = torch.randint(-2, 3, (M, 8 * cout), generator=g).to(torch.bfloat16)
        w32 = [torch.randint(-1, 2, s, generator=g).float() for s in [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]]
        cs = [torch.randint(1, 4, (n,), generator=g).float() for n in [cout] * 4 + [2 * cout]]
        bias = torch.randint(-2, 3, (cout,), generator=g).float()
    else:
        x = torch.randn(M, 8 * cin, generator=g).to(torch.bfloat16)
        dy = torch.randn(M, 8 * cout, generator=g).to(torch.bfloat16)
        w32 = [torch.randn(s, generator=g) * 0.1 for s in [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]]
        cs = [torch.rand(n, generator=g) + 0.5 for n in [cout] * 4 + [2 * cout]]
        bias = torch.randn(cout, generator=g)
    return x.to(DEV), dy.to(DEV), [w.to(DEV) for w in w32], [c.to(DEV) for c in cs], bias.to(DEV)


def _wgrad(x, dy, cin, cout, mask, rps, w32=None, cs=None, bias=None, want_bias=True):
    """(dw5, dcs5 or None, dbias) of one launch + finish; mask None = the plain entry."""
    from octic_vits_amd import ops
    M = x.shape[0]
    ss = None if mask is None else torch.tensor(mask, dtype=torch.float32, device=DEV)
    dw, dcs, dbias = ops.linear_wgrad(ops.pview(x, cin), ops.pview(dy, cout), M, cin, cout, x.dtype, x, w32=w32, cs5=cs,
                                      bias=bias if cs is not None else None, want_bias=want_bias, may_defer=False,
                                      sample_scale=ss, rows_per_sample=rps)
    torch.cuda.synchronize()
    return dw, dcs, dbias


def _same(a, b, what):
    dwa, dca, dba = a
    dwb, dcb, dbb = b
    for i in range(5):
        assert torch.equal(dwa[i], dwb[i]), (what, "dw", i)
        if dca is not None:
            assert torch.equal(dca[i], dcb[i]), (what, "dcs", i)
    if dba is not None:
        assert torch.equal(dba, dbb), (what, "dbias")


def _reference(x, dy, cin, cout, w32, cs, bias):
    """float64: (G5, |dY|^T |X| per group, column sums of dY_A1, of |dY_A1|), then (dw5, dcs5 or None, dbias)."""
    xs, ys = _groups(x.double(), cin), _groups(dy.double(), cout)
    G = [yg.t() @ xg for xg, yg in zip(xs, ys)]
    A = [yg.abs().t() @ xg.abs() for xg, yg in zip(xs, ys)]
    ysum, yabs = ys[0].sum(0), ys[0].abs().sum(0)
    if cs is None:
        return G, A, ysum, yabs, (G, None, ysum)
    dw = [c.double()[:, None] * g for c, g in zip(cs, G)]
    dcs = [(w.double() * g).sum(1) for w, g in zip(w32, G)]
    dcs[0] = dcs[0] + bias.double() * ysum
    return G, A, ysum, yabs, (dw, dcs, cs[0].double() * ysum)


def _bounds(x, dy, cin, cout, w32, cs, bias):
    """Elementwise bounds that hold for ANY grouping of the f32 sums: derived, not measured.  G[n, k] is a sum of n_rows
    products of bf16 numbers (8 + 8 significand bits: exact in f32) accumulated in f32 in some order.  Each of the at most
    n_rows - 1 additions, the MFMA's internal ones included, errs by at most 2^-23 of a partial sum (one ulp, which also covers
    an adder that truncates) whose size is at most A = (|dY|^T |X|)[n, k], so one grouping lies within n 2^-23 A of the float64
    product and two groupings within  2 n 2^-23 A  of each other - the bound used for both comparisons.  The column sums of
    dY_A1 likewise with A = sum |dY_A1|.  The finish then computes  dw = cs G  (one more rounding),
    dcs = sum_k W G + bias ysum  (K products and additions in f32: K 2^-23 of sum |W| |G| + |bias| |ysum|) and
    dbias = cs ysum  (one rounding); the bounds on G and ysum go through these linear maps."""
    M = x.shape[0]
    G, A, ysum, yabs, ref = _reference(x, dy, cin, cout, w32, cs, bias)
    n = [M] * 4 + [2 * M]
    bG = [2 * nn * U * a for nn, a in zip(n, A)]
    bY = 2 * M * U * yabs
    if cs is None:
        return ref, (bG, None, bY)
    bdw = [c.double()[:, None] * b + U * d.abs() for c, b, d in zip(cs, bG, ref[0])]
    bdcs = [(w.double().abs() * b).sum(1) + w.shape[1] * U * (w.double().abs() * (a + b)).sum(1) for w, b, a in zip(w32, bG, A)]
    bdcs[0] = bdcs[0] + bias.double().abs() * bY + w32[0].shape[1] * U * bias.double().abs() * (yabs + bY)
    bdb = cs[0].double() * bY + U * ref[2].abs()
    return ref, (bdw, bdcs, bdb)


def _within(got, ref, bound, what):
    for name, g, r, b in zip(("dw", "dcs", "dbias"), got, ref, bound):
        if g is None:
            continue
        g, r, b = (list(v) if isinstance(v, (list, tuple)) else [v] for v in (g, r, b))
        for i, (gi, ri, bi) in enumerate(zip(g, r, b)):
            err = (gi.double() - ri).abs()
            assert bool((err <= bi).all()), (what, name, i, float(err.max()), float(bi.min()))


def _zero_dropped(dy, mask, rps):
    out = dy.clone()
    out[~_row_keep(mask, rps)] = 0
    return out


CASES = [(cin, cout, B, rps) for cin, cout in SHAPES for B in (4, 6) for rps in (5, 33, 257)]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "bias+scale"])
@pytest.mark.parametrize("cin,cout,B,rps", CASES)
def test_exact_operands_equal_the_unmasked_launch_and_float64(cin, cout, B, rps, scaled):
    from octic_vits_amd import _lib
    M = B * rps
    assert _lib.plan("octic_linear_d8_wgrad_plan", M, cin, cout, _lib.BF16)[0] == _lib.WGRAD_RING
    x, dy, w32, cs, bias = _problem(cin, cout, M, True)
    kw = dict(w32=w32, cs=cs, bias=bias) if scaled else {}
    for name, mask in _masks(B).items():
        dyz = _zero_dropped(dy, mask, rps)
        got = _wgrad(x, dyz, cin, cout, mask, rps, **kw)
        _same(got, _wgrad(x, dyz, cin, cout, None, 0, **kw), (name, "unmasked launch"))
        ref = _reference(x, dyz, cin, cout, w32, cs if scaled else None, bias)[4]
        for nm, g, r in zip(("dw", "dcs", "dbias"), got, ref):
            if g is None:
                continue
            for i, (gi, ri) in enumerate(zip(*((g, r) if isinstance(g, list) else ([g], [r])))):
                assert torch.equal(gi.double(), ri), (name, nm, i)
        _same(got, _wgrad(x, dyz, cin, cout, mask, rps, **kw), (name, "second launch"))          # 4: determinism


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "bias+scale"])
@pytest.mark.parametrize("cin,cout,B,rps", CASES)
def test_random_operands_stay_within_the_regrouping_bound(cin, cout, B, rps, scaled):
    M = B * rps
    x, dy, w32, cs, bias = _problem(cin, cout, M, False)
    kw = dict(w32=w32, cs=cs, bias=bias) if scaled else {}
    for name, mask in _masks(B).items():
        dyz = _zero_dropped(dy, mask, rps)
        ref, bound = _bounds(x, dyz, cin, cout, w32, cs if scaled else None, bias)
        got = _wgrad(x, dyz, cin, cout, mask, rps, **kw)
        _within(got, ref, bound, name)
        _same(got, _wgrad(x, dyz, cin, cout, mask, rps, **kw), (name, "second launch"))


def _dead_rows(M, mask, rps, pair):
    """Token rows of the steps (32 LDS rows from the group's row 0; pair rows = token >> 1) that touch no kept sample."""
    rows = 2 * M if pair else M
    dead = torch.zeros(M, dtype=torch.bool)
    for t in range((rows + 31) // 32):
        toks = sorted({(mm >> 1) if pair else mm for mm in range(32 * t, min(32 * t + 32, rows))})
        if not any(mask[tok // rps] != 0 for tok in toks):
            dead[toks] = True
    return dead.to(DEV)


@pytest.mark.parametrize("cin,cout,B,rps", CASES)
def test_dead_steps_are_not_read(cin, cout, B, rps):
    M = B * rps
    x, dy, w32, cs, bias = _problem(cin, cout, M, False)
    hit = 0
    for name, mask in _masks(B).items():
        dyz = _zero_dropped(dy, mask, rps)
        clean = _wgrad(x, dyz, cin, cout, mask, rps, w32=w32, cs=cs, bias=bias)
        xp = x.clone()
        dead_a, dead_e = _dead_rows(M, mask, rps, False), _dead_rows(M, mask, rps, True)
        xp[:, :4 * cin][dead_a] = float("nan")
        xp[:, 4 * cin:][dead_e] = float("nan")
        hit += int(dead_a.sum()) + int(dead_e.sum())
        _same(_wgrad(xp, dyz, cin, cout, mask, rps, w32=w32, cs=cs, bias=bias), clean, name)
    assert hit > 0 or rps == 5                                       # (at 5 rows per sample only long runs of drops kill a step)


@pytest.mark.parametrize("cin,cout", SHAPES)
def test_edge_masks(cin, cout):
    from octic_vits_amd import _lib
    for B, rps in ((4, 5), (6, 33), (4, 257)):
        M = B * rps
        x, dy, w32, cs, bias = _problem(cin, cout, M, False)
        nobody = [0.0] * B
        dw, dcs, dbias = _wgrad(torch.full_like(x, float("nan")), torch.zeros_like(dy), cin, cout, nobody, rps, w32=w32, cs=cs,
                                bias=bias)
        for t in list(dw) + list(dcs) + [dbias]:
            assert bool((t == 0).all()), (B, rps)
    # one kept sample of 5 rows among 64: one or two live steps per group for the plan's splits
    B, rps = 64, 5
    M = B * rps
    assert _lib.plan("octic_linear_d8_wgrad_plan", M, cin, cout, _lib.BF16)[2] >= 2
    x, dy, w32, cs, bias = _problem(cin, cout, M, True)
    for b in (0, 10, 63):
        mask = [0.0] * B
        mask[b] = KEEP
        dyz = _zero_dropped(dy, mask, rps)
        got = _wgrad(x, dyz, cin, cout, mask, rps, w32=w32, cs=cs, bias=bias)
        _same(got, _wgrad(x, dyz, cin, cout, None, 0, w32=w32, cs=cs, bias=bias), b)


def test_fallbacks_are_the_plain_launches():
    from octic_vits_amd import _lib
    B, rps = 4, 33
    M = B * rps
    mask = [KEEP, 0.0, 0.0, KEEP]
    x, dy, w32, cs, bias = _problem(160, 160, M, False)
    plain = _wgrad(x, dy, 160, 160, None, 0)
    # f32 operands and a 96-wide shape run the tiled kernel, which computes every row (dy is NOT zeroed here)
    xf, dyf = x.float(), dy.float()
    assert _lib.plan("octic_linear_d8_wgrad_plan", M, 160, 160, _lib.F32)[0] == _lib.WGRAD_TILED
    _same(_wgrad(xf, dyf, 160, 160, mask, rps, want_bias=False), _wgrad(xf, dyf, 160, 160, None, 0, want_bias=False), "f32")
    x96, dy96 = _problem(96, 96, M, False)[:2]
    assert _lib.plan("octic_linear_d8_wgrad_plan", M, 96, 96, _lib.BF16)[0] == _lib.WGRAD_TILED
    _same(_wgrad(x96, dy96, 96, 96, mask, rps, want_bias=False), _wgrad(x96, dy96, 96, 96, None, 0, want_bias=False), "96-wide")
    # a NULL mask through the _skip entry is the plain entry
    from octic_vits_amd import ops
    import ctypes
    L = _lib.lib()
    splits = _lib.plan("octic_linear_d8_wgrad_plan", M, 160, 160, _lib.BF16)[2]
    n = L.octic_linear_d8_wgrad_workspace_bytes(160, 160, splits) // 4
    ws = [torch.zeros(n, device=DEV) for _ in range(2)]
    xv, dyv = ops.pview(x, 160), ops.pview(dy, 160)
    ops.check(L.octic_linear_d8_wgrad(ctypes.byref(xv), ctypes.byref(dyv), M, 160, 160, _lib.BF16, ops._p(ws[0]), splits, None))
    ops.check(L.octic_linear_d8_wgrad_skip(ctypes.byref(xv), ctypes.byref(dyv), M, 160, 160, _lib.BF16, ops._p(ws[1]), splits,
                                           None, 0, None))
    torch.cuda.synchronize()
    assert torch.equal(ws[0], ws[1]) and bool((ws[0] != 0).any())
    assert plain[0][0].abs().max() > 0


# ---- 7: a training step -----------------------------------------------------------------------------------------------
def _model():
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.vit import Layer_scale_init_Block
    torch.manual_seed(0)
    return OcticVisionTransformer(octic_block_layers=Layer_scale_init_BlockD8, standard_block_layers=Layer_scale_init_Block,
                                  img_size=224, patch_size=14, num_classes=10, embed_dim=1280, depth=2, num_heads=16,
                                  qkv_bias=True, init_scale=0.1, drop_path_rate=0.5, octic_equi_break_layer=1).cuda()


@functools.lru_cache(maxsize=None)
def _steps():
    """(off, on, eager on, captured on) as (loss, {name: p.grad}), and {name: float64 bound} from the operands of the off step's
    octic weight-gradient calls (functional._linear_d8_grads is hooked for that one step).  The first two steps run without
    the optimizer, which rewrites the gradient buffers it is handed: their p.grad are the gradients.  The last two are whole
    steps, compared with each other only: capture(warmup=1) runs one eager step and records the next, so the eager side is
    two steps under the same eight masks."""
    import octic_vits_amd.d8_layers as L
    import octic_vits_amd.functional as OF
    from octic_vits_amd.train import Trainer, synthetic_batch
    B = 4
    cache = {}
    for k in range(16):
        g = torch.Generator().manual_seed(500 + k)
        cache[k] = (torch.bernoulli(torch.full((B,), 0.5), generator=g) * KEEP).to(DEV)
    calls = [0]

    def source(Bn, keep, device):
        k = calls[0] % 16
        calls[0] += 1
        return cache[k]

    x, y = synthetic_batch(B, 10, DEV, seed=3, img_size=224)
    before, grads_fn = OF.LINEAR_WGRAD_SKIP_DROPPED, OF._linear_d8_grads
    seen = []

    def hooked(ctx, x_, g_, w5, cs32, b32, *a, **k):
        seen.append((x_.detach().clone(), g_.detach().clone(), list(w5), cs32, b32, ctx.lin[0], ctx.lin[1]))
        return grads_fn(ctx, x_, g_, w5, cs32, b32, *a, **k)

    out, bounds = [], {}
    L.drop_path_mask_source = source
    try:
        for on, whole, captured in ((False, False, False), (True, False, False), (True, True, False), (True, True, True)):
            OF.LINEAR_WGRAD_SKIP_DROPPED = on
            calls[0] = 0
            tr = Trainer(_model(), lr=1e-3)
            names = {id(p): n for n, p in tr.raw_model.named_parameters()}
            if captured:
                loss = tr.capture(x, y, warmup=1).replay(x, y).detach().clone()
            else:
                if not whole:
                    tr.optimizer.step = lambda *a, **k: None
                if not on:
                    OF._linear_d8_grads = hooked
                try:
                    if whole:
                        tr.step(x, y)
                    loss = tr.step(x, y).detach().clone()
                finally:
                    OF._linear_d8_grads = grads_fn
            torch.cuda.synchronize()
            out.append((loss, {n: p.grad.detach().clone() for n, p in tr.raw_model.named_parameters() if p.grad is not None}))
            if not on:
                assert len(seen) == 4                                # qkv, proj, fc1, fc2 of the one octic block
                for x_, g_, w5, cs32, b32, cin, cout in seen:
                    xs, gs = x_.reshape(-1, 8 * cin), g_.reshape(-1, 8 * cout)
                    w32 = [w.detach().float() for w in w5]
                    scaled = cs32 is not None
                    _, (bdw, bdcs, bdb) = _bounds(xs, gs, cin, cout, w32, list(cs32) if scaled else None,
                                                  b32 if b32 is not None else torch.zeros(cout, device=DEV))
                    prefix = names[id(w5[0])][:-len(".lin_A1.weight")]
                    for w, b in zip(w5, bdw):
                        bounds[names[id(w)]] = b
                    if b32 is not None:
                        bounds[prefix + ".lin_A1.bias"] = bdb
                    if scaled:
                        block, layer = prefix.rsplit(".", 2)[0], prefix.rsplit(".", 1)[1]
                        gamma = block + (".gamma_1" if layer == "proj" else ".gamma_2")
                        for irrep, b in zip(("A1", "A2", "B1", "B2", "E"), bdcs):
                            bounds[f"{gamma}.alpha_{irrep}"] = b
                seen.clear()
    finally:
        L.drop_path_mask_source = None
        OF.LINEAR_WGRAD_SKIP_DROPPED = before
        OF._linear_d8_grads = grads_fn
    return out, bounds


def test_training_step_moves_only_the_octic_gradients_and_within_the_bound():
    (off, on, _, _), bounds = _steps()
    assert torch.equal(off[0], on[0]) and bool(torch.isfinite(on[0]).all())
    assert set(off[1]) == set(on[1]) and len(on[1]) > 20
    assert len(bounds) == 4 * 5 + 4 + 2 * 5 and set(bounds) <= set(on[1])    # 20 weights, 4 biases, 10 layer scales
    moved, worst = 0, 0.0
    for n in on[1]:
        if n not in bounds:
            assert torch.equal(on[1][n], off[1][n]), n
            continue
        err = (on[1][n].double() - off[1][n].double()).abs()
        b = bounds[n].reshape(err.shape)
        worst = max(worst, float((err / b.clamp_min(1e-300)).max()))
        print(f"{n}: max |on - off| {float(err.max()):.3e}, largest share of its bound {float((err / b.clamp_min(1e-300)).max()):.3e}")
        assert bool((err <= b).all()), (n, float(err.max()))
        moved += int((err > 0).any())
    print(f"octic gradients that moved: {moved} of {len(bounds)}; largest |on - off| / bound {worst:.3e}")


def test_captured_training_step_equals_the_eager_one():
    (_, _, on, cap), _ = _steps()
    assert torch.equal(on[0], cap[0])
    assert set(on[1]) == set(cap[1])
    for n in on[1]:
        assert torch.equal(on[1][n], cap[1][n]), n
