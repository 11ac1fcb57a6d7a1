"""Input rows of the DINO / iBOT head calls on the HIP engine (csrc/dino_head.hip, functional.HeadRowsFn, ssl.HEAD_HIP): the
gather against the index arithmetic it replaces (new_zeros + index_select + copy_ + cat) and the scatter against autograd of that
composition, bitwise - the rows are distinct, so no sum is reordered - and the DINOv2 step with the switch on against off."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape, dtype=torch.float32):
    return torch.randn(*shape, generator=g, device="cuda").to(dtype)


# ------------------------------------------------------------------------------------------------------- head rows
def _stock_rows(local_cls, x_norm, R, idx, upperbound):
    """ssl_meta_arch.py:226-267: local cls | global cls | masked patch tokens | zero pad."""
    sp = x_norm[:, 1 + R:]
    buf = sp.new_zeros(upperbound, sp.shape[-1])
    buf[:idx.shape[0]].copy_(torch.index_select(sp.flatten(0, 1), dim=0, index=idx))
    return torch.cat([local_cls, x_norm[:, 0], buf], dim=0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("T,D", [(5, 128), (197, 128), (5, 1280), (197, 1280)])
@pytest.mark.parametrize("R", [0, 4], ids=["noreg", "reg4"])
def test_head_rows_equal_the_index_arithmetic_bitwise(dtype, T, D, R):
    from octic_vits_amd import functional as OF
    B, P = 4, T - 1
    upperbound = min(B * P, 40)
    g = _gen(T * D + R)
    for n_masked in (0, 1, upperbound):
        idx = torch.randperm(B * P, generator=g, device="cuda")[:n_masked].sort().values
        leaf_l = _randn(g, 6, D, dtype=dtype).requires_grad_(True)
        leaf_g = _randn(g, B, 1 + R + P, D, dtype=dtype).requires_grad_(True)
        cot = _randn(g, 6 + B + upperbound, D, dtype=dtype)
        want = _stock_rows(leaf_l, leaf_g, R, idx, upperbound)
        want.backward(cot)
        gl, gg = leaf_l.grad.clone(), leaf_g.grad.clone()
        leaf_l.grad = leaf_g.grad = None
        srcs = (leaf_l, leaf_g[:, 0], leaf_g[:, 1 + R:])
        specs = ((None, 0), (None, 6), (idx, 6 + B))
        assert OF.head_rows_ok(6 + B + upperbound, specs, srcs)
        got = OF.HeadRowsFn.apply(6 + B + upperbound, specs, *srcs)
        assert got.dtype == dtype and torch.equal(got, want.detach())
        pad = got[6 + B + n_masked:]
        pad = pad.detach()
        assert pad.numel() == 0 or (float(pad.abs().max()) == 0.0 and not bool(torch.signbit(pad).any()))   # +0
        got.backward(cot)
        assert torch.equal(leaf_l.grad, gl) and torch.equal(leaf_g.grad, gg), (n_masked,)


def test_head_rows_refuses_what_the_kernel_does_not_take():
    from octic_vits_amd import functional as OF, ops
    x = torch.randn(4, 9, 64, device="cuda")
    idx = torch.arange(3, device="cuda")
    assert not OF.head_rows_ok(8, ((idx.int(), 0),), (x,))
    assert not OF.head_rows_ok(8, ((None, 0),), (x[..., :60],))
    assert not OF.head_rows_ok(8, ((None, 0),), (x.cpu(),))
    out = torch.empty(8, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.head_rows([(x, idx, 6)], out)                                    # rows 6 .. 8 of an 8-row buffer
    with pytest.raises(ValueError):
        ops.head_rows([(x[:, 0], None, 0), (x, idx, 2)], out)                # overlapping segments
    # indices outside the source are never dereferenced: +0 rows
    bad = torch.tensor([1, 4 * 9, -1], device="cuda")
    got = ops.head_rows([(x, bad, 0)], out)
    assert torch.equal(got[0], x.flatten(0, 1)[1]) and float(got[1:].abs().max()) == 0.0


def _timed(fn):
    from octic_vits_amd import ops
    ops.KERNEL_TIMER.enable()
    try:
        out = fn()
        names = {r[0] for r in ops.KERNEL_TIMER.records}
    finally:
        ops.KERNEL_TIMER.disable()
        ops.KERNEL_TIMER.records = []
    return out, names


# ------------------------------------------------------------------------------------------------------- the step
def _arch(seed=0, **kw):
    from octic_vits_amd import ssl as S
    from test_ssl_gpu import DIM, KW, _product_backbone
    torch.manual_seed(seed)
    return S.SSLMetaArch(_product_backbone, DIM, koleo_loss_weight=0.1, **{**KW, **kw}).cuda().train()


def _images(B, seed):
    from octic_vits_amd import ssl as S
    random.seed(seed)
    g = torch.Generator().manual_seed(seed)
    gc, lc = torch.randn(2 * B, 3, 32, 32, generator=g), torch.randn(2 * B, 3, 16, 16, generator=g)
    im = S.collate(gc, lc, (0.1, 0.5), 0.5, 64, S.MaskingGenerator((8, 8), max_num_patches=32))
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in im.items()}


@pytest.mark.parametrize("autocast", [True, False], ids=["bf16", "f32"])
@pytest.mark.parametrize("centering", ["centering", "sinkhorn_knopp"])
def test_step_with_the_switch_on_against_off(centering, autocast):
    """forward_backward on the small architecture of tests/test_koleo_gpu.py's step tests: every loss term within 5e-2 (the bf16
    rule of tests/test_ssl_gpu.py) of the run with the switch off, every gradient finite, and the kernels launched exactly when
    the switch is on - for float32 sources (no autocast) as well as under bf16 autocast."""
    import contextlib
    from octic_vits_amd import ssl as S

    def run(on):
        arch = _arch(centering=centering)
        S.HEAD_HIP = on
        try:
            with (torch.autocast("cuda", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()):
                (out, names) = _timed(lambda: arch.forward_backward(_images(4, 3), teacher_temp=0.05))
        finally:
            S.HEAD_HIP = True
        grads = [p.grad for p in arch.student.parameters() if p.grad is not None]
        assert len(grads) > 60 and all(bool(torch.isfinite(g).all()) for g in grads)
        return {k: float(v.detach()) for k, v in out.items()}, names

    on, names_on = run(True)
    off, names_off = run(False)
    print(on, off)
    assert set(on) == set(off)
    for k in off:
        assert on[k] == pytest.approx(off[k], rel=5e-2, abs=5e-3), k
    for k in ("head_rows_kernel<gather", "head_rows_kernel<scatter"):
        assert any(n.startswith(k) for n in names_on), (k, names_on)
        assert not any(n.startswith(k) for n in names_off), (k, names_off)


@pytest.mark.parametrize("separate", [False, True], ids=["shared_head", "separate_ibot_head"])
def test_two_trainer_steps(separate):
    from octic_vits_amd import ssl as S
    arch = _arch(ibot_separate_head=separate)
    tr = S.SSLTrainer(arch, lr=1e-3)
    images = _images(4, 3)
    for _ in range(2):
        out, names = _timed(lambda: tr.step(images, teacher_temp=0.05, momentum=0.9))
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        assert any(n.startswith("head_rows_kernel<gather") for n in names) and any(n.startswith("head_rows_kernel<scatter") for n in names)
    assert all(bool(torch.isfinite(p).all()) for p in arch.parameters())
