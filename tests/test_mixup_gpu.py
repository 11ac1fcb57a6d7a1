"""csrc/mixup.hip, octic_vits_amd.mixup, Trainer(mixup=...) and train.evaluate on the GPU.

Yardstick for everything that is not bitwise (the `within` rule of tests/test_seg_gpu.py): the reference is the float64 torch
composition on the device; the kernel's maximum error, normalised by the largest float64 magnitude of that quantity, may be at
most 2x the error of the stock f32 torch composition on the same inputs, plus one f32 ulp (2^-23).  The stock composition is
the restatement of timm's Mixup in tests/golden/mixup_case.py and nn.BCEWithLogitsLoss / F.cross_entropy."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mixup_case
from octic_vits_amd.mixup import MixParams, Mixup, mix_bce_loss, mix_images, mix_targets

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23


def within(what, got, stock, ref):
    """max |got - ref| / max |ref|  <=  2 max |stock - ref| / max |ref| + one f32 ulp; prints the three figures first."""
    ref = ref.double()
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max()) / scale
    stock_err = float((stock.double() - ref).abs().max()) / scale
    print(f"{what}: kernel {err:.3e}  stock f32 {stock_err:.3e}  bar {2 * stock_err + ULP:.3e}")
    assert err <= 2 * stock_err + ULP, (what, err, stock_err)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _table(p):
    return torch.from_numpy(p.table()).to(DEV)


# ------------------------------------------------------------------------------------------------ images
IMAGE_SHAPES = [(2, 3, 8, 8), (4, 3, 7, 30), (8, 3, 32, 32), (6, 1, 33, 36), (4, 3, 224, 224)]


def _hand_tables(B, H, W):
    """Tables whose rows walk through: untouched, full-image box, empty box, a box on the top and left borders, one on the
    bottom and right borders, a box whose columns are no multiples of 4, two blends (a blend ignores its box).  Partners:
    B-1-i, except row 0, which points at row 1."""
    xl, xh = (5, W - 3) if W >= 12 else (1, W - 2)
    kinds = [
        (1.0, False, (0, 0, 0, 0)),
        (0.0, True, (0, H, 0, W)),
        (0.7, True, (2, 2, 3, 3)),
        (0.5, True, (0, H // 2, 0, W // 2 + 1)),
        (0.5, True, (H // 2, H, W // 3, W)),
        (0.6, True, (1, H - 1, xl, xh)),
        (0.3, False, (0, 0, 0, 0)),
        (0.81, False, (1, H, 1, W)),
    ]
    tables = []
    for start in range(0, len(kinds), B):
        rows = [kinds[(start + i) % len(kinds)] for i in range(B)]
        partner = np.arange(B - 1, -1, -1)
        partner[0] = 1
        tables.append(MixParams(partner, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
    return tables


def _check_images(x, p, out):
    B = x.shape[0]
    blend_rows = []
    for i in range(B):
        j, lam = int(p.partner[i]), float(p.lam[i])
        yl, yh, xl, xh = (int(v) for v in p.box[i])
        if lam == 1.0:
            assert torch.equal(out[i], x[i]), i
        elif p.cut[i]:
            want = x[i].clone()
            want[:, yl:yh, xl:xh] = x[j][:, yl:yh, xl:xh]
            assert torch.equal(out[i], want), (i, p.box[i])
        else:
            blend_rows.append(i)
    if not blend_rows:
        return False
    idx = torch.tensor(blend_rows, device=DEV)
    par = torch.from_numpy(p.partner[blend_rows].astype(np.int64)).to(DEV)
    lam = torch.from_numpy(p.lam[blend_rows]).to(DEV).view(-1, 1, 1, 1)
    ref = x[idx].double() * lam.double() + x[par].double() * (1 - lam.double())
    stock = x[idx] * lam + x[par] * (1 - lam)
    within(f"mix_images blend {tuple(x.shape)}", out[idx], stock, ref)
    return True


@pytest.mark.parametrize("shape", IMAGE_SHAPES)
def test_mix_images_hand_written_tables(shape):
    B, C, H, W = shape
    x = torch.randn(shape, generator=_gen(B + W), device=DEV)
    kept = x.clone()
    blends = 0
    for p in _hand_tables(B, H, W):
        out = mix_images(x, _table(p))
        assert torch.equal(x, kept)                     # out of place
        blends += _check_images(x, p, out)
    assert blends
    # into a caller's buffer (the captured step's input), and identity rows for a table that says nothing
    buf = torch.full_like(x, float("nan"))
    assert mix_images(x, _table(p), out=buf) is buf and torch.equal(buf, out)
    assert torch.equal(mix_images(x, _table(MixParams.identity(B))), x)


def test_mix_images_unaligned_pointers_take_the_element_path():
    B, C, H, W = 4, 3, 8, 36                            # W % 4 == 0 but the buffers start 4 bytes off a 16-byte boundary
    n = B * C * H * W
    flat, oflat = torch.randn(n + 1, generator=_gen(3), device=DEV), torch.empty(n + 1, device=DEV)
    x, out = flat[1:].view(B, C, H, W), oflat[1:].view(B, C, H, W)
    assert x.data_ptr() % 16 == 4
    for p in _hand_tables(B, H, W):
        mix_images(x, _table(p), out=out)
        _check_images(x, p, out)
        assert torch.equal(out, mix_images(x.clone(), _table(p)))  # the vector path gives the same bits


def test_mix_images_rejects_bad_arguments():
    x = torch.randn(4, 3, 8, 8, device=DEV)
    t = _table(MixParams.identity(4))
    with pytest.raises(RuntimeError, match="shape"):
        mix_images(x, t, out=x)                         # in place = overlapping
    with pytest.raises(ValueError):
        mix_images(x.half(), t)
    with pytest.raises(ValueError):
        mix_images(x, t[:2])
    # a table that points outside the batch mixes nothing
    bad = MixParams(np.array([7, -1, 2, 1]), [0.5, 0.5, 2.0, float("nan")], [False] * 4, np.zeros((4, 4)))
    assert torch.equal(mix_images(x, _table(bad)), x)


# ------------------------------------------------------------------------------------------------ whole apply
def _soft_targets_f64(y, lam, nc, s):
    off = s / nc
    on = 1. - s + off
    lam = torch.from_numpy(lam.astype(np.float64)).to(DEV).view(-1, 1)
    oh = lambda t: torch.full((len(t), nc), off, dtype=torch.float64, device=DEV).scatter_(1, t.view(-1, 1), on)
    return oh(y) * lam + oh(y.flip(0)) * (1 - lam)


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
@pytest.mark.parametrize("shape,nc,smoothing", [((8, 3, 32, 32), 10, 0.0), ((4, 3, 7, 30), 1001, 0.1), ((6, 1, 33, 36), 1000, 0.0)])
def test_apply_matches_the_timm_restatement(mode, shape, nc, smoothing):
    B = shape[0]
    kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, mode=mode, label_smoothing=smoothing, num_classes=nc)
    x = torch.randn(shape, generator=_gen(B), device=DEV)
    y = torch.randint(0, nc, (B,), generator=_gen(B + 1), device=DEV)
    ours, ref = Mixup(**kw), mixup_case.RefMixup(**kw)
    mixed_any = cut_any = False
    for seed in range(6):
        np.random.seed(seed)
        got_x, got_t = ours(x, y)
        np.random.seed(seed)
        got_xb, got_b = ours.apply(x, y, binarize=True)
        np.random.seed(seed)
        stock_x, stock_t = ref(x.clone(), y)
        lam, cut, box = mixup_case.normalised(ref.last)
        np.random.seed(seed)
        ref_x, _ = ref(x.double(), y)
        assert torch.equal(got_x, got_xb)
        within(f"apply images {mode} {shape} seed {seed}", got_x, stock_x, ref_x)
        for i in np.nonzero(cut | (lam == 1))[0]:       # pasted / untouched samples: bit for bit
            assert torch.equal(got_x[i], stock_x[i]), (seed, i)
        within(f"apply soft targets {mode} {nc} seed {seed}", got_t, stock_t, _soft_targets_f64(y, lam, nc, smoothing))
        assert torch.equal(got_b, stock_t.gt(0).float())
        if smoothing > 0:
            assert bool((got_b == 1).all())             # the reference's quirk: smoothing makes every binarised entry 1
        mixed_any |= bool((lam != 1).any())
        cut_any |= bool(cut.any())
    assert mixed_any and cut_any


def test_mix_targets_chunks_and_bad_labels():
    B, nc = 8, 1000
    p = Mixup(0.8, 1.0, mode="elem", num_classes=nc, rng=np.random.RandomState(1)).draw(B, 32, 32)
    t = _table(p)
    y = torch.randint(0, nc, (B,), generator=_gen(5), device=DEV)
    for binarize in (False, True):
        whole = mix_targets(y, t, nc, on=0.9001, off=0.0001, binarize=binarize)
        assert whole.shape == (B, nc)
        for row0, rows in ((0, 4), (4, 4), (0, 3), (3, 5), (7, 1)):
            part = mix_targets(y, t, nc, on=0.9001, off=0.0001, binarize=binarize, row0=row0, rows=rows)
            assert torch.equal(part, whole[row0:row0 + rows]), (row0, rows)
    # a label outside [0, nc): its one-hot row is all `off`; the partner's class still shows
    y2 = y.clone()
    y2[0], y2[B - 1] = nc, -1
    got = mix_targets(y2, t, nc, on=1.0, off=0.0)
    assert float(got[0].sum()) == 0.0 and float(got[B - 1].sum()) == 0.0
    y2[B - 1] = 3
    got = mix_targets(y2, t, nc, on=1.0, off=0.0)
    lam0 = float(p.lam[0])
    assert float(got[0].sum()) == float(got[0, 3]) == pytest.approx(1 - lam0, abs=1e-7)


# ------------------------------------------------------------------------------------------------ the loss
def _bce_problem(rows, nc, dtype, ld=None, seed=0):
    ld = ld or nc
    logits = (3 * torch.randn(rows, ld, generator=_gen(seed), device=DEV)).to(dtype)      # the columns past nc are padding
    y = torch.randint(0, nc, (rows,), generator=_gen(seed + 1), device=DEV)
    y[0] = y[rows - 1]                                   # a pair with the same class
    p = Mixup(0.8, 1.0, mode="elem", num_classes=nc, rng=np.random.RandomState(seed)).draw(rows, 32, 32)
    return logits, y, p


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,nc,ld", [(2, 10, None), (8, 1000, None), (16, 1001, None), (8, 1000, 1024)])
@pytest.mark.parametrize("binarize", [True, False])
def test_mix_bce_loss_value_and_gradient(dtype, rows, nc, ld, binarize):
    logits, y, p = _bce_problem(rows, nc, dtype, ld, seed=rows)
    t = _table(p)
    on, off = (1.0, 0.0) if binarize else (0.9 + 0.1 / nc, 0.1 / nc)
    lam32 = torch.from_numpy(p.lam).to(DEV).view(-1, 1)
    oh = lambda lab, dt: torch.full((rows, nc), off, dtype=dt, device=DEV).scatter_(1, lab.view(-1, 1), on)
    t32 = oh(y, torch.float32) * lam32 + oh(y.flip(0), torch.float32) * (1. - lam32)
    t64 = oh(y, torch.float64) * lam32.double() + oh(y.flip(0), torch.float64) * (1. - lam32.double())
    if binarize:
        t32, t64 = t32.gt(0).float(), t64.gt(0).double()
    assert torch.equal(mix_targets(y, t, nc, on=on, off=off, binarize=binarize), t32)

    def run(fn, x0):                                     # the leaf keeps the row stride; the loss sees its first nc columns
        x = x0.detach().clone().requires_grad_(True)
        loss = fn(x[:, :nc])
        loss.backward()
        return loss.detach(), x.grad[:, :nc]

    kern = lambda x: mix_bce_loss(x, y, t, on=on, off=off, binarize=binarize)
    got_l, got_g = run(kern, logits)
    stock_l, stock_g = run(lambda x: torch.nn.BCEWithLogitsLoss()(x.float(), t32), logits)
    ref_l, ref_g = run(lambda x: torch.nn.BCEWithLogitsLoss()(x, t64), logits.double())
    assert got_l.dtype == torch.float32 and got_g.dtype == dtype and got_g.shape == (rows, nc)
    tag = f"{'bf16' if dtype == torch.bfloat16 else 'f32'} {rows}x{nc} ld {ld} {'binarised' if binarize else 'soft'}"
    within(f"mix_bce value {tag}", got_l.view(1), stock_l.view(1), ref_l.view(1))
    within(f"mix_bce dlogits {tag}", got_g, stock_g, ref_g)
    # bitwise repeatable; an upstream gradient scales dlogits exactly
    l2, g2 = run(kern, logits)
    assert torch.equal(l2, got_l) and torch.equal(g2, got_g)
    _, gq = run(lambda x: kern(x) * 0.25, logits)
    assert torch.equal(gq, got_g * 0.25)
    # chunks: the rows of a chunk read their partners' labels in the whole batch; 1 / (rows nc) is the only difference
    if rows >= 4:
        h = rows // 2
        for row0 in (0, h):
            lc, gc = run(lambda x: mix_bce_loss(x, y, t, on=on, off=off, binarize=binarize, row0=row0), logits[row0:row0 + h])
            assert torch.equal(gc, got_g[row0:row0 + h] * 2), row0
            ref_c = torch.nn.BCEWithLogitsLoss()(logits[row0:row0 + h, :nc].double(), t64[row0:row0 + h])
            stock_c = torch.nn.BCEWithLogitsLoss()(logits[row0:row0 + h, :nc].float(), t32[row0:row0 + h])
            within(f"mix_bce chunk value {tag} row0 {row0}", lc.view(1), stock_c.view(1), ref_c.view(1))


# ------------------------------------------------------------------------------------------------ the trainer
KW = dict(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=4, num_heads=2,
          mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=2)
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=10)


def _model():
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(0)
    return OcticVisionTransformer(**KW).cuda()


def _batches(n, B=8, seed=100):
    g = _gen(seed)
    return [(torch.randn(B, 3, 32, 32, generator=g, device=DEV), torch.randint(0, 10, (B,), generator=g, device=DEV))
            for _ in range(n)]


def _same_weights(ta, tb):
    for (n, pa), pb in zip(ta.raw_model.named_parameters(), tb.raw_model.parameters()):
        assert torch.equal(pa, pb), n
    for ea, eb in zip(ta.optimizer.ema_state(), tb.optimizer.ema_state()):
        assert torch.equal(ea, eb)


def test_trainer_unfused_equals_a_plain_trainer_fed_mixed_batches():
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(7), **MIX), fused_loss=False)
    tb = Trainer(_model(), lr=1e-3)
    mix = Mixup(rng=np.random.RandomState(7), **MIX)
    la, lb = [], []
    for x, y in _batches(4):
        la.append(float(ta.step(x, y)))
        lb.append(float(tb.step(*mix.apply(x, y, binarize=True))))
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)
    with pytest.raises(TypeError, match="int64 class labels"):
        ta.step(x, torch.zeros(8, 10, device=DEV))
    with pytest.raises(RuntimeError, match="GPU only"):
        ta.step(x, y.cpu())


@pytest.mark.parametrize("accum,steps", [(1, 8), (2, 3)])
def test_trainer_fused_captured_step_equals_eager(accum, steps):
    """Eager against captured with the mix and the fused loss inside the graph; the replays are issued back to back (the host
    runs ahead of the device: more replays than the table ring has slots), nothing is read before the end."""
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, accum_steps=accum, mixup=Mixup(rng=np.random.RandomState(11), **MIX))
    tb = Trainer(_model(), lr=1e-3, accum_steps=accum, mixup=Mixup(rng=np.random.RandomState(11), **MIX))
    batches = _batches(steps + 1, seed=200 + accum)
    gs = tb.capture(*batches[0], warmup=2)
    for _ in range(2):
        ta.step(*batches[0])
    lb = [gs.replay(x, y).clone() for x, y in batches[1:]]
    la = [ta.step(x, y) for x, y in batches[1:]]
    la, lb = [float(v) for v in la], [float(v) for v in lb]
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)


def test_trainer_fused_first_loss_agrees_with_the_unfused_one():
    from octic_vits_amd.train import Trainer
    x, y = _batches(1, seed=300)[0]
    seen = {}
    losses = {}
    for fused in (True, False):
        tr = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(5), **MIX), fused_loss=fused)
        hook = tr.raw_model.head.register_forward_hook(lambda m, i, o, k=fused: seen.__setitem__(k, o.detach().clone()))
        losses[fused] = tr.step(x, y).clone()
        hook.remove()
    assert torch.equal(seen[True], seen[False])          # the same mixed batch went through the same weights
    logits = seen[True]
    _, t = Mixup(rng=np.random.RandomState(5), **MIX).apply(x, y, binarize=True)
    ref = torch.nn.BCEWithLogitsLoss()(logits.double(), t.double())
    stock = torch.nn.BCEWithLogitsLoss()(logits.float(), t)
    assert torch.equal(stock, losses[False])
    within("trainer first loss, fused", losses[True].view(1), stock.view(1), ref.view(1))


# ------------------------------------------------------------------------------------------------ evaluate
def _distinct_rank_labels(logits):
    """A label per row whose logit ties with no other of the row, at rank 0, 2 or 7 in turn (or the next untied rank): top-k
    membership is then the same for torch.topk and for the kernel's count of strictly greater logits."""
    labels = []
    for i, row in enumerate(logits.float().cpu()):
        vals, idx = row.sort(descending=True)
        r = (0, 2, 7)[i % 3]
        while r < len(vals) and ((r > 0 and vals[r - 1] == vals[r]) or (r + 1 < len(vals) and vals[r + 1] == vals[r])):
            r += 1
        assert r < len(vals)
        labels.append(int(idx[r]))
    return torch.tensor(labels, device=DEV)


def test_evaluate_matches_the_torch_composition():
    from octic_vits_amd.train import evaluate
    model = _model().eval()
    g = _gen(9)
    images = [torch.randn(n, 3, 32, 32, generator=g, device=DEV) for n in (8, 8, 5)]
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        logits = [model(x).float() for x in images]
    labels = [_distinct_rank_labels(l) for l in logits]
    batches = list(zip(images, labels))
    n = 21
    all_logits, all_labels = torch.cat(logits), torch.cat(labels)
    top = all_logits.topk(5, 1, True, True)[1]
    c1 = int((top[:, :1] == all_labels.view(-1, 1)).sum())
    c5 = int((top == all_labels.view(-1, 1)).sum())
    assert 0 < c1 < c5 < n
    ref = F.cross_entropy(all_logits.double(), all_labels, reduction="sum") / n
    stock = sum(F.cross_entropy(l, y, reduction="sum") for l, y in zip(logits, labels)) / n
    for graphed in (True, False):
        got = evaluate(model, batches, graphed=graphed)
        assert set(got) == {"loss", "acc1", "acc5"}
        assert got["acc1"] == 100.0 * c1 / n and got["acc5"] == 100.0 * c5 / n, (got, c1, c5)
        within(f"evaluate loss graphed={graphed}", torch.tensor([got["loss"]], dtype=torch.float64), stock.view(1).cpu(),
               ref.view(1).cpu())
    # the graph and the eager launches run the same kernels: bitwise on the full batches
    assert evaluate(model, batches[:2], graphed=True) == evaluate(model, batches[:2], graphed=False)
    with pytest.raises(ValueError):
        evaluate(model, [(images[0], labels[0].float())])
