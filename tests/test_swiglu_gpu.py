"""DINOv2's SwiGLU FFN on the MI355X: the gate kernels of csrc/swiglu.hip through ``ops`` (rounding pinned bit for bit where the
sigmoid is exactly 1, extremes of bf16's range, float64 oracles on random inputs, column sums, refusals, the dispatcher op),
``vit.SwiGLUFFNFused.forward_fused`` and ``vit.NestedTensorBlock`` with it against the eager bf16 composition, torch.compile,
the fused optimizer's bf16 copies, the reference goldens, and the unchanged ``ffn_layer="mlp"`` path."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import baseline_cases as BC
import cases
import swiglu_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ROWS = [1, 3, 7, 257, 1030, 2100]       # 2100: 9 rows per row block - the two-row trip and the single-row tail in one lane
WIDTHS = [8, 344, 512, 520]             # 1, 43, 64, 65 eight-wide column chunks: below, at, just above one 64-lane group


def _ops():
    from octic_vits_amd import ops
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ulp_bf16(v):
    """Spacing of bf16 at |v| (float64 tensor): 2^(floor(log2 |v|) - 7), the smallest normal's below that."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7)


def _oracle(x12, ga):
    """The kernels' formulas in float64 on the bf16 values (CPU)."""
    H = x12.shape[1] // 2
    x1, x2 = x12[:, :H].double().cpu(), x12[:, H:].double().cpu()
    s = 1.0 / (1.0 + torch.exp(-x1))
    a = x1 * s * x2
    if ga is None:
        return a
    g = ga.double().cpu()
    return a, g * x2 * s * (1 + x1 * (1 - s)), g * x1 * s


def _rand(rows, H, seed):
    g = torch.Generator().manual_seed(seed)
    x12 = (3 * torch.randn(rows, 2 * H, generator=g)).to(BF)
    ga = (3 * torch.randn(rows, H, generator=g)).to(BF)
    return x12.to(DEV), ga.to(DEV)


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("H", WIDTHS)
@pytest.mark.parametrize("rows", ROWS)
def test_gate_kernels_against_float64(rows, H):
    """Forward within 1 bf16 ulp of the rounded oracle (the f32 evaluation error, ~1e-6 relative, is far below the half ulp
    2^-9: only rounding ties can flip); backward within ulp_bf16(oracle) + 2^-18 |ga x2| (|ga x1| for the value half): the
    second term is the absolute f32 error of the O(1) factor silu', which cancels near x1 = -1.28.  Column sums: the float64
    sums of the kernel's own stored dx12 within rows 2^-24 sum|dx12| per column, bitwise equal across two launches, [2H] in
    w12.bias order."""
    o = _ops()
    x12, ga = _rand(rows, H, 1000 * rows + H)
    a = o.swiglu_fwd(x12, H)
    dx, db = o.swiglu_bwd(x12, ga, want_colsum=True)
    dx_b, db_b = o.swiglu_bwd(x12, ga, want_colsum=True)
    dx_n, none = o.swiglu_bwd(x12, ga, want_colsum=False)
    assert a.shape == (rows, H) and a.dtype == BF and dx.shape == (rows, 2 * H) and dx.dtype == BF
    assert db.shape == (2 * H,) and db.dtype == torch.float32 and none is None
    wa, w1, w2 = _oracle(x12, ga)
    wab = wa.to(BF).double()
    err = (a.double().cpu() - wab).abs()
    assert bool((err <= _ulp_bf16(wab)).all()), float((err / _ulp_bf16(wab)).max())
    x1, x2, g = x12[:, :H].double().cpu(), x12[:, H:].double().cpu(), ga.double().cpu()
    for got, want, mag in ((dx[:, :H], w1, (g * x2).abs()), (dx[:, H:], w2, (g * x1).abs())):
        err = (got.double().cpu() - want).abs()
        tol = _ulp_bf16(want) + 2.0 ** -18 * mag
        assert bool((err <= tol).all()), float((err / tol).max())
    assert torch.equal(_bits(dx), _bits(dx_b)) and torch.equal(_bits(dx), _bits(dx_n))
    assert torch.equal(db, db_b)                                     # fixed summation order
    stored = dx.double().cpu()
    bound = rows * 2.0 ** -24 * stored.abs().sum(0)
    assert bool(((db.double().cpu() - stored.sum(0)).abs() <= bound + 1e-300).all())


def test_rounding_is_nearest_even_bit_for_bit_where_the_sigmoid_is_one():
    """For x1 >= 17 the f32 sigmoid is exactly 1 (1 + exp(-17) == 1.0f: tests/test_swiglu_host.py), and a product of two bf16
    values is exact in f32: a == bf16(x1 x2), dx1 == bf16(ga x2), dx2 == bf16(ga x1) bit for bit."""
    o = _ops()
    rows, H = 257, 520
    g = torch.Generator().manual_seed(17)
    x1 = (17 + 87 * torch.rand(rows, H, generator=g)).to(BF)
    assert float(x1.min()) >= 17 and float(x1.max()) <= 104
    x2 = (3 * torch.randn(rows, H, generator=g)).to(BF)
    ga = (3 * torch.randn(rows, H, generator=g)).to(BF)
    x12 = torch.cat((x1, x2), dim=1).to(DEV)
    a = o.swiglu_fwd(x12, H).cpu()
    dx, _ = o.swiglu_bwd(x12, ga.to(DEV), want_colsum=False)
    dx = dx.cpu()
    assert torch.equal(_bits(a), _bits((x1.float() * x2.float()).to(BF)))
    assert torch.equal(_bits(dx[:, :H]), _bits((ga.float() * x2.float()).to(BF)))
    assert torch.equal(_bits(dx[:, H:]), _bits((ga.float() * x1.float()).to(BF)))


def test_extreme_inputs_never_give_nan():
    o = _ops()
    X1 = [0.0, 88.0, -88.0, 104.0, -104.0, 3e38, -3e38]
    combos = [(a, b, c) for a in X1 for b in (1.0, -1.0, 0.5) for c in (1.0, -2.0)]
    H = 8
    x1 = torch.tensor([c[0] for c in combos]).view(-1, 1).expand(-1, H).to(BF)
    x2 = torch.tensor([c[1] for c in combos]).view(-1, 1).expand(-1, H).to(BF)
    ga = torch.tensor([c[2] for c in combos]).view(-1, 1).expand(-1, H).to(BF).contiguous()
    x12 = torch.cat((x1, x2), dim=1).to(DEV)
    a = o.swiglu_fwd(x12, H).cpu()
    dx, _ = o.swiglu_bwd(x12, ga.to(DEV), want_colsum=False)
    dx = dx.cpu()
    d1, d2 = dx[:, :H], dx[:, H:]
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(dx).any())
    zero = (x1 == 0)[:, 0]
    assert bool((a[zero] == 0).all()) and bool((d2[zero] == 0).all())
    assert torch.equal(_bits(d1[zero]), _bits((0.5 * ga.float() * x2.float()).to(BF)[zero]))
    low = (x1.float() <= -104)[:, 0]
    for t in (a, d1, d2):
        assert float(t[low].float().abs().max()) < 1e-30
    high = (x1.float() >= 88)[:, 0]
    assert int(zero.sum()) == 6 and int(low.sum()) == 12 and int(high.sum()) == 18
    assert torch.equal(_bits(a[high]), _bits((x1.float() * x2.float()).to(BF)[high]))
    assert torch.equal(_bits(d1[high]), _bits((ga.float() * x2.float()).to(BF)[high]))
    assert torch.equal(_bits(d2[high]), _bits((ga.float() * x1.float()).to(BF)[high]))      # (-2 * 3e38 = -inf: correctly infinite)
    assert bool(torch.isinf(d2[high]).any())


@pytest.mark.parametrize("rows,H", [(7, 344), (257, 520)])
def test_strided_operands_leave_the_canary_columns_alone(rows, H):
    """ld12 > 2H, ldg > H, lda > H, ldd > 2H: views of wider buffers filled with a canary."""
    o = _ops()
    x12, ga = _rand(rows, H, 5)
    want_a = o.swiglu_fwd(x12, H)
    want_dx, want_db = o.swiglu_bwd(x12, ga)
    can = 777.0
    xb = torch.full((rows, 2 * H + 24), can, dtype=BF, device=DEV)
    gb = torch.full((rows, H + 16), can, dtype=BF, device=DEV)
    ab = torch.full((rows, H + 40), can, dtype=BF, device=DEV)
    db_ = torch.full((rows, 2 * H + 32), can, dtype=BF, device=DEV)
    xv, gv, av, dv = xb[:, 16:16 + 2 * H], gb[:, 8:8 + H], ab[:, 24:24 + H], db_[:, 8:8 + 2 * H]
    xv.copy_(x12), gv.copy_(ga)
    assert o.swiglu_fwd(xv, H, out=av) is av
    dx, db = o.swiglu_bwd(xv, gv, out=dv)
    assert dx is dv
    assert torch.equal(_bits(av), _bits(want_a)) and torch.equal(_bits(dv), _bits(want_dx)) and torch.equal(db, want_db)
    for buf, lo, hi in ((ab, 24, 24 + H), (db_, 8, 8 + 2 * H), (xb, 16, 16 + 2 * H), (gb, 8, 8 + H)):
        assert bool((buf[:, :lo] == can).all()) and bool((buf[:, hi:] == can).all())


def test_refusals_raise_and_leave_the_outputs_untouched():
    o = _ops()
    can = 777.0

    def outs(rows, H, pad=0):
        return (torch.full((rows, H + pad), can, dtype=BF, device=DEV), torch.full((rows, 2 * H + pad), can, dtype=BF, device=DEV))

    def refused(x12, ga, H, a, dx):
        with pytest.raises(RuntimeError, match="octic HIP call failed"):
            o.swiglu_fwd(x12, H, out=a)
        with pytest.raises(RuntimeError, match="octic HIP call failed"):
            o.swiglu_bwd(x12, ga, out=dx)
        torch.cuda.synchronize()
        assert bool((a == can).all()) and bool((dx == can).all())

    # H = 12
    x12, ga = torch.zeros(4, 24, dtype=BF, device=DEV), torch.zeros(4, 12, dtype=BF, device=DEV)
    refused(x12, ga, 12, *outs(4, 12))
    # an odd row stride (input side, then output side)
    wide = torch.zeros(4, 33, dtype=BF, device=DEV)
    refused(wide[:, :32], torch.zeros(4, 16, dtype=BF, device=DEV), 16, *outs(4, 16))
    a, dx = outs(4, 16, pad=1)
    refused(torch.zeros(4, 32, dtype=BF, device=DEV), torch.zeros(4, 16, dtype=BF, device=DEV), 16, a[:, :16], dx[:, :32])
    assert bool((a == can).all()) and bool((dx == can).all())
    # a base pointer one element off
    flat = torch.zeros(4 * 32 + 8, dtype=BF, device=DEV)
    refused(flat[1:1 + 4 * 32].view(4, 32), torch.zeros(4, 16, dtype=BF, device=DEV), 16, *outs(4, 16))
    # rows = 0: empty tensors, no launch
    e12, eg = torch.zeros(0, 32, dtype=BF, device=DEV), torch.zeros(0, 16, dtype=BF, device=DEV)
    assert o.swiglu_fwd(e12, 16).shape == (0, 16)
    dx0, db0 = o.swiglu_bwd(e12, eg)
    assert dx0.shape == (0, 32) and db0.shape == (32,) and not bool(db0.any())
    with pytest.raises(ValueError):
        o.swiglu_fwd(torch.zeros(4, 32, device=DEV), 16)                 # f32 rows


def test_dispatcher_op_passes_opcheck_and_equals_the_kernels():
    from octic_vits_amd import dispatch  # noqa: F401
    o = _ops()
    x12, ga = _rand(33, 72, 3)
    torch.library.opcheck(torch.ops.octic.swiglu, (x12.view(3, 11, 144).clone().requires_grad_(True),))
    torch.library.opcheck(torch.ops.octic.swiglu, (x12.clone(),))
    x = x12.clone().requires_grad_(True)
    a = torch.ops.octic.swiglu(x)
    (gx,) = torch.autograd.grad(a, x, ga)
    assert torch.equal(_bits(a), _bits(o.swiglu_fwd(x12, 72)))
    assert torch.equal(_bits(gx), _bits(o.swiglu_bwd(x12, ga, want_colsum=False)[0]))


def test_kernels_run_under_the_kernel_timer_with_their_byte_counts():
    o = _ops()
    x12, ga = _rand(257, 512, 4)
    o.KERNEL_TIMER.enable()
    try:
        o.swiglu_fwd(x12, 512)
        o.swiglu_bwd(x12, ga)
        agg = o.KERNEL_TIMER._agg()
    finally:
        o.KERNEL_TIMER.disable()
        o.KERNEL_TIMER.records = []
    assert agg["swiglu_fwd_kernel"]["bytes"] == 257 * 512 * 6 and agg["swiglu_bwd_kernel"]["bytes"] == 257 * 512 * 10


# ------------------------------------------------------------------------------------------------ 2. module
def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm()) / max(float(b.double().norm()), 1e-12)


def _assert_rule(got, want, ref32, yard, what):
    """The rule of tests/test_baselines_gpu.py: output within 5e-2 of scale; every gradient within max(3e-2, 2 x the CPU
    model's own bf16-autocast distance from its f32 run) in relative L2.  got / want: the engine and the eager bf16
    composition on the GPU; ref32 / yard: the CPU composition in f32 and under bf16 autocast.  Each: (outputs, {name: grad})."""
    for a, b in zip(got[0], want[0]):
        scale = max(1.0, float(b.float().abs().max()))
        assert float((a.float() - b.float()).abs().max()) <= 5e-2 * scale, what
    bad = []
    for n in want[1]:
        bound = max(3e-2, 2.0 * _rel(yard[1][n], ref32[1][n]))
        rel = _rel(got[1][n], want[1][n])
        if rel > bound:
            bad.append(f"{n}: {rel:.4f} > {bound:.4f}")
    assert set(got[1]) == set(want[1]) and not bad, f"{what}: " + "; ".join(bad)


def _compose(ffn, y, xres, gamma, rs, norm, cots, device, autocast, fused=False):
    """xres + rs gamma ffn(y) (+ the next norm) as plain torch ops - or through forward_fused - with gradients of every input."""
    leaves = {"y": y, "xres": xres}
    if gamma is not None:
        leaves["gamma"] = gamma
    leaves = {k: v.detach().to(device).clone().requires_grad_(True) for k, v in leaves.items()}
    rsd = None if rs is None else rs.to(device)
    for p in list(ffn.parameters()) + ([] if norm is None else list(norm.parameters())):
        p.grad = None
    with torch.autocast(device, dtype=BF, enabled=autocast):
        if fused:
            out = ffn.forward_fused(leaves["y"], leaves["xres"], leaves.get("gamma"), rsd, BF, next_norm=norm)
            outs = list(out) if norm is not None else [out]
        else:
            f = ffn(leaves["y"]).float()
            if gamma is not None:
                f = f * leaves["gamma"]
            if rsd is not None:
                f = f * rsd.view(-1, 1, 1)
            outs = [leaves["xres"] + f]
            if norm is not None:
                outs.append(norm(outs[0]))
    sum((o.float() * c.to(device)).sum() for o, c in zip(outs, cots)).backward()
    grads = {k: v.grad.detach().float().cpu() for k, v in leaves.items()}
    for n, p in list(ffn.named_parameters()) + ([] if norm is None else [("norm." + k, v) for k, v in norm.named_parameters()]):
        grads[n] = p.grad.detach().float().cpu()
    return [o.detach().float().cpu() for o in outs], grads


@pytest.mark.parametrize("variant", ["plain", "nobias", "nogamma", "nextnorm", "dropped"])
@pytest.mark.parametrize("dim,H", [(192, 512), (128, 344)])
def test_forward_fused_equals_the_eager_composition(dim, H, variant):
    """(192, 512): all four GEMMs on csrc/dense_gemm.hip; (128, 344): the library-GEMM fallback around the HIP gate kernels.
    "dropped": a per-sample stochastic-depth factor with one dropped sample (the kernels may skip its rows)."""
    from octic_vits_amd import vit
    o = _ops()
    tag = f"swiglu.{dim}.{variant}"
    ffn = vit.SwiGLUFFNFused(dim, 4 * dim, bias=variant != "nobias")
    cases.fill_parameters(ffn, salt=tag + ".")
    assert ffn.w3.in_features == H
    norm = None
    if variant == "nextnorm":
        norm = nn.LayerNorm(dim, eps=1e-6)
        cases.fill_parameters(norm, salt=tag + ".norm.")
    B, T = 4, 17
    y32 = cases.randn(tag + ".y", B, T, dim)
    xres = cases.randn(tag + ".x", B, T, dim)
    gamma = None if variant == "nogamma" else 0.5 + 0.2 * cases.randn(tag + ".g", dim)
    rs = torch.tensor([4 / 3, 0.0, 4 / 3, 4 / 3]) if variant == "dropped" else None
    cots = [cases.randn(tag + ".c0", B, T, dim), cases.randn(tag + ".c1", B, T, dim)]
    ref32 = _compose(ffn, y32, xres, gamma, rs, norm, cots, "cpu", False)
    yard = _compose(ffn, y32, xres, gamma, rs, norm, cots, "cpu", True)
    ffn, norm = ffn.to(DEV), (None if norm is None else norm.to(DEV))
    yb = y32.to(BF)                                   # forward_fused takes y in the compute dtype
    want = _compose(ffn, yb, xres, gamma, rs, norm, cots, DEV, True)
    o.KERNEL_TIMER.enable()
    try:
        got = _compose(ffn, yb, xres, gamma, rs, norm, cots, DEV, True, fused=True)
        names = set(o.KERNEL_TIMER._agg())
    finally:
        o.KERNEL_TIMER.disable()
        o.KERNEL_TIMER.records = []
    assert {"swiglu_fwd_kernel", "swiglu_bwd_kernel"} <= names, sorted(names)
    hip = [n for n in names if n.startswith("dense_nt_kernel")]
    lib = [n for n in names if n.startswith("library_gemm<fwd") or n.startswith("library_gemm<dgrad")]
    if H == 512:
        assert ffn.rows_ok(yb.to(DEV)) and hip and not lib, sorted(names)
    else:
        assert not ffn.rows_ok(yb.to(DEV)) and lib and not hip, sorted(names)
    _assert_rule(got, want, ref32, yard, tag)
    # inference (the DINOv2 teacher): same values, nothing saved
    with torch.no_grad(), torch.autocast(DEV, dtype=BF):
        out = ffn.forward_fused(yb.to(DEV), xres.to(DEV), None if gamma is None else gamma.to(DEV),
                                None if rs is None else rs.to(DEV), BF, next_norm=norm)
    out = out[0] if norm is not None else out
    assert out.grad_fn is None and torch.equal(out.float().cpu(), got[0][0])


# ------------------------------------------------------------------------------------------------ 3. blocks
def _block(drop_path=0.0, seed="blk"):
    from octic_vits_amd import vit
    blk = vit.NestedTensorBlock(dim=192, num_heads=3, qkv_bias=True, ffn_layer=vit.SwiGLUFFNFused, init_values=1.0,
                                drop_path=drop_path)
    cases.fill_parameters(blk, salt=f"swiglu.{seed}.")
    return blk


def _eager_block(blk, x, masks, cot, device, autocast):
    """block.py:86-111 as plain module calls with the given per-sample stochastic-depth factors (None: no drop)."""
    blk = blk.to(device)
    for p in blk.parameters():
        p.grad = None
    x = x.detach().to(device).clone().requires_grad_(True)
    m1, m2 = (None if m is None else m.to(device).view(-1, 1, 1) for m in masks)
    with torch.autocast(device, dtype=BF, enabled=autocast):
        f = blk.ls1(blk.attn(blk.norm1(x))).float()
        x1 = x + (f if m1 is None else f * m1)
        f = blk.ls2(blk.mlp(blk.norm2(x1))).float()
        out = x1 + (f if m2 is None else f * m2)
    (out.float() * cot.to(device)).sum().backward()
    grads = {"x": x.grad.detach().float().cpu()}
    grads.update({n: p.grad.detach().float().cpu() for n, p in blk.named_parameters()})
    return [out.detach().float().cpu()], grads


def _engine_block(blk, x, cot, fn=None):
    for p in blk.parameters():
        p.grad = None
    x = x.detach().to(DEV).clone().requires_grad_(True)
    with torch.autocast(DEV, dtype=BF):
        out = (blk if fn is None else fn)(x)
    (out.float() * cot.to(DEV)).sum().backward()
    grads = {"x": x.grad.detach().float().cpu()}
    grads.update({n: p.grad.detach().float().cpu() for n, p in blk.named_parameters()})
    return [out.detach().float().cpu()], grads, out


@pytest.mark.parametrize("mode", ["eval", "train_drop_path_0.05"])
def test_block_equals_the_eager_composition(mode, monkeypatch):
    """Eval: the engine path (DenseSwigluFn is the node).  Training with drop_path 0.05: block.py:100-104's per-sample masks, as
    vit.NestedTensorBlock draws them (recorded here and handed to the composition)."""
    from octic_vits_amd import vit
    train = mode != "eval"
    blk = _block(drop_path=0.05 if train else 0.0).train(train)
    B = 16 if train else 4
    x, cot = cases.randn("swiglu.blk.x", B, 17, 192), cases.randn("swiglu.blk.c", B, 17, 192)
    drawn = []

    def drop_path(self, t):                           # vit.DropPath.forward, keeping the mask
        if self.drop_prob == 0. or not self.training:
            return t
        keep = 1 - self.drop_prob
        mask = t.new_empty((t.shape[0],) + (1,) * (t.ndim - 1)).bernoulli_(keep).div_(keep)
        drawn.append(mask.detach().float().view(-1).cpu())
        return t * mask
    monkeypatch.setattr(vit.DropPath, "forward", drop_path)
    torch.manual_seed(3)
    got_out, got_g, out = _engine_block(blk.to(DEV), x, cot)
    if train:
        assert len(drawn) == 2
    else:
        assert not drawn and "DenseSwigluFn" in type(out.grad_fn).__name__
    masks = drawn if train else (None, None)
    want = _eager_block(blk, x, masks, cot, DEV, True)
    cpu = copy.deepcopy(blk).cpu()
    ref32 = _eager_block(cpu, x, masks, cot, "cpu", False)
    yard = _eager_block(cpu, x, masks, cot, "cpu", True)
    _assert_rule((got_out, got_g), want, ref32, yard, mode)


def test_block_subset_stochastic_depth_fused_and_eager_pick_the_same_samples():
    """drop_path 0.3 in training (block.py:113-140): vit.SUBSET_FUSED True and False under one seed."""
    from octic_vits_amd import vit
    blk = _block(drop_path=0.3).to(DEV).train()
    x0, cot = cases.randn("swiglu.sub.x", 10, 17, 192), cases.randn("swiglu.sub.c", 10, 17, 192)

    def run(fused):
        vit.SUBSET_FUSED = fused
        torch.manual_seed(123)
        torch.cuda.manual_seed(123)
        o_, g_, _ = _engine_block(blk, x0, cot)
        return o_[0], g_

    try:
        oe, ge = run(False)
        of, gf = run(True)
    finally:
        vit.SUBSET_FUSED = True
    changed = (oe - x0).flatten(1).abs().amax(1) > 0
    assert 0 < int(changed.sum()) <= 10
    assert torch.equal(changed, (of - x0).flatten(1).abs().amax(1) > 0)          # the same samples
    assert float((oe - of).abs().max()) <= 5e-2 * max(1.0, float(oe.abs().max()))
    for n in ge:
        assert _rel(gf[n], ge[n]) <= 3e-2, (n, _rel(gf[n], ge[n]))


@pytest.mark.parametrize("mode", ["eval", "train", "train_drop_path_0.3"])
def test_block_ragged_pass_equals_the_set_by_set_loop(mode):
    """Two crop sets (2 x 197 and 4 x 37 tokens: a 224 and a 96 crop at patch 16, as in test_baselines_gpu.py) as ONE row tensor
    against the loop over the sets.  drop_path 0.3: the kept rows travel through row maps (rows_to) or gather / scatter
    (vit.ROW_MAPS) - the same subsets under one seed."""
    from octic_vits_amd import functional as OF
    from octic_vits_amd import ragged as R
    from octic_vits_amd import vit
    sub = mode.endswith("0.3")
    blk = _block(drop_path=0.3 if sub else 0.0, seed="rag").to(DEV).train(mode != "eval")
    sets = [(2, 197), (4, 37)]
    xs = [cases.randn(f"swiglu.rag.x{i}", b, t, 192) for i, (b, t) in enumerate(sets)]
    cs = [cases.randn(f"swiglu.rag.c{i}", b, t, 192) for i, (b, t) in enumerate(sets)]
    rows = torch.cat([x.reshape(1, -1, 192) for x in xs], dim=1)
    crow = torch.cat([c.reshape(1, -1, 192) for c in cs], dim=1)

    def ragged(row_maps=True):
        rag = R.Ragged(sets)
        prev, OF.RAGGED, vit.ROW_MAPS = OF.RAGGED, rag, row_maps
        try:
            torch.manual_seed(7)
            torch.cuda.manual_seed(7)
            if sub:                                   # the subsets of both branches, with their row maps (as the model loop draws them)
                rag.draw_perms(2, DEV, [max(int(b * 0.7), 1) for b, _ in sets])
            out = _engine_block(blk, rows, crow, fn=lambda t: blk._ragged(t, rag))
            assert out[2] is not None
            return out[:2]
        finally:
            OF.RAGGED, vit.ROW_MAPS = prev, True

    got = ragged()
    if sub:
        want = ragged(row_maps=False)
        assert not torch.equal(got[0][0], rows) and bool(((got[0][0] - rows).abs().amax(-1) == 0).any())
    else:
        for p in blk.parameters():
            p.grad = None
        leaves = [x.to(DEV).clone().requires_grad_(True) for x in xs]
        with torch.autocast(DEV, dtype=BF):
            outs = [blk(t) for t in leaves]
        sum((o_.float() * c.to(DEV)).sum() for o_, c in zip(outs, cs)).backward()
        grads = {"x": torch.cat([t.grad.reshape(1, -1, 192) for t in leaves], dim=1).float().cpu()}
        grads.update({n: p.grad.detach().float().cpu() for n, p in blk.named_parameters()})
        want = ([torch.cat([o_.detach().reshape(1, -1, 192) for o_ in outs], dim=1).float().cpu()], grads)
    assert float((got[0][0] - want[0][0]).abs().max()) <= 5e-2 * max(1.0, float(want[0][0].abs().max()))
    for n in want[1]:
        assert _rel(got[1][n], want[1][n]) <= 3e-2, (n, _rel(got[1][n], want[1][n]))


def test_block_compiles_with_zero_graph_breaks_and_equals_eager():
    from octic_vits_amd import dispatch  # noqa: F401
    import torch._dynamo as dynamo
    blk = _block(seed="cmp").to(DEV).train()
    x, cot = cases.randn("swiglu.cmp.x", 4, 17, 192), cases.randn("swiglu.cmp.c", 4, 17, 192)
    eo, eg, _ = _engine_block(blk, x, cot)
    dynamo.reset()
    comp = torch.compile(blk, backend="aot_eager", fullgraph=True)          # any graph break raises
    co, cg, _ = _engine_block(blk, x, cot, fn=comp)
    def run(t):
        with torch.autocast(DEV, dtype=BF):
            return blk(t)
    info = dynamo.explain(run)(x.to(DEV))
    dynamo.reset()
    targets = {str(n.target) for gm in info.graphs for n in gm.graph.nodes if n.op == "call_function"}
    assert info.graph_break_count == 0 and any("octic.swiglu" in t for t in targets), sorted(targets)
    cpu = copy.deepcopy(blk).cpu()
    ref32 = _eager_block(cpu, x, (None, None), cot, "cpu", False)
    yard = _eager_block(cpu, x, (None, None), cot, "cpu", True)
    _assert_rule((co, cg), (eo, eg), ref32, yard, "compiled")


# ------------------------------------------------------------------------------------------------ 4. models
def _small_model(**kw):
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    spec = dict(img_size=28, patch_size=14, embed_dim=192, depth=2, num_heads=3, ffn_layer="swiglufused", init_values=1.0)
    spec.update(kw)
    return DinoVisionTransformer(**spec)


def test_fused_optimizer_keeps_the_bf16_copies_current():
    """One fused-optimizer step through train.Trainer on a 2-block SwiGLU model: the forward that follows runs on the bf16
    copies the optimizer wrote (w12 / w3 listed by train.library_gemm_layers) and equals a fresh model loaded with the updated
    state dict; the step moved the output by far more than the tolerance, so a stale copy would show."""
    from octic_vits_amd.train import Trainer
    m = _small_model()
    cases.fill_parameters(m, salt="swiglu.opt.")
    m.mask_token.requires_grad_(False)                # (not reached without masks: the fused optimizer wants every gradient)
    m = m.to(DEV)
    x = cases.randn("swiglu.opt.img", 4, 3, 28, 28).to(DEV)
    y = (cases.randn("swiglu.opt.t", 4, 192) > 0).float().to(DEV)

    def fwd(model):
        model.eval()
        with torch.no_grad(), torch.autocast(DEV, dtype=BF):
            return model(x).float()

    before = fwd(m)
    tr = Trainer(m, lr=1e-2, tuned_gemms=False)
    m.train()
    tr.step(x, y)
    ffn = m.blocks[0].mlp
    assert ffn._c1.static and ffn._c2.static          # adopted from the optimizer's update pass
    got = fwd(m)
    fresh = _small_model()
    fresh.load_state_dict(m.state_dict())
    want = fwd(fresh.to(DEV))
    scale = max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= 1e-3 * scale
    assert float((before - want).abs().max()) >= 2e-2 * scale


@pytest.mark.parametrize("name", list(SC.CASES))
def test_golden_cases_on_the_gpu(name):
    """f32 within 1e-3 of scale, bf16 autocast (the engine path) within 5e-2 of scale of the reference's CPU outputs."""
    m = SC.build(_small_model_any, name)
    SC.check_golden(SC.run_model(m, name, device=DEV), tol=1e-3)
    SC.check_golden(SC.run_model(m, name, device=DEV, autocast=True), tol=5e-2)


def _small_model_any(**kw):
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    return DinoVisionTransformer(**kw)


def test_mlp_ffn_is_unchanged():
    """ffn_layer="mlp": DenseMlpFn is still the node a vit_large-style block runs, and an existing baseline golden still
    passes from here."""
    from functools import partial
    from octic_vits_amd import vit
    from octic_vits_amd.dinov2_vit import DinoVisionTransformer
    torch.manual_seed(0)
    blk = partial(vit.NestedTensorBlock, attn_class=vit.MemEffAttention)(dim=256, num_heads=4, qkv_bias=True,
                                                                         init_values=1e-5).to(DEV).train()
    assert type(blk.mlp) is vit.Mlp
    with torch.autocast(DEV, dtype=BF):
        out = blk(torch.randn(2, 17, 256, device=DEV))
    assert type(out.grad_fn).__name__.startswith("DenseMlpFn")
    name = "baseline_dino"
    got = BC.run_dino_case(lambda **kw: DinoVisionTransformer(**kw), name, device=DEV)
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        if want[k].size:
            scale = max(1.0, float(np.abs(want[k]).max()))
            assert float(np.abs(got[k] - want[k]).max()) <= 1e-3 * scale, k
