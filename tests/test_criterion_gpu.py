"""The criterion kernels of csrc/mixup.hip on the GPU: octic_mix_ce (soft-target / label-smoothing / plain cross entropy) and
octic_cosub_bce (the four BCE terms of --cosub), their autograd wrappers in octic_vits_amd.mixup, and
Trainer(loss=..., smoothing=..., cosub=...).

Oracle: stock torch in float64 on the CPU - F.cross_entropy with probability targets (or class labels and label_smoothing), and
the four-term expression with F.binary_cross_entropy_with_logits; the targets are a numpy restatement of timm's mixup_target with
its three f32 roundings (tests/test_criterion_host.py checks in float64 that this oracle is the label-smoothing cross entropy
on identity-table targets).

Yardstick (the rule of tests/test_sinkhorn_gpu.py and `within` of tests/test_mixup_gpu.py): the stock f32 torch composition runs
on the same device inputs in the same test; the kernel's error against float64 may be at most twice that composition's error plus
a floor of FLOOR_ULPS f32 ulps of the quantity's largest magnitude (for the cases where the composition happens to be exact).
Where the composition itself overflows (the bf16-max logits) the floor alone is the bar.  bf16 gradients are compared with the
float64 gradient rounded to bf16 and may be one bf16 ulp off.  Every check prints its figures before it asserts (pytest -s).

Code paths of mix_ce_kernel in C (csrc/mixup.hip): rows of up to 2048 classes live in 8 registers per thread, up to 24576 in 96,
longer rows are re-read by every pass - 2048 / 2049 and 24576 / 24577 are the edges, 21841 (ImageNet-21k) the large resident
shape, 50000 one well past the last edge.  A slot is 1024 f32 / 2048 bf16 elements: 1000 / 1001, 2048 / 2049 straddle it."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from octic_vits_amd import ops
from octic_vits_amd.mixup import (MixParams, Mixup, cosub_bce_loss, mix_bce_loss, mix_ce_loss, mix_images, mix_targets,
                                  smoothing_on_off)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23
FLOOR_ULPS = 4
BF16_MAX = 3.3895313892515355e38


def within(what, got, stock, ref, floor_ulps=FLOOR_ULPS):
    """max |got - ref| / max |ref|  <=  2 max |stock - ref| / max |ref| + floor_ulps f32 ulps; all on the CPU in float64."""
    ref = ref.detach().double().cpu()
    got, stock = got.detach().double().cpu(), stock.detach().double().cpu()
    scale = max(float(ref.abs().max()), 1e-300)
    err = float((got - ref).abs().max()) / scale
    stock_err = float((stock - ref).abs().max()) / scale
    bar = floor_ulps * ULP + (2 * stock_err if np.isfinite(stock_err) else 0.0)
    print(f"{what}: kernel {err:.3e}  stock f32 {stock_err:.3e}  bar {bar:.3e}")
    assert np.isfinite(err) and err <= bar, (what, err, stock_err, bar)
    return err, stock_err


def bf16_close(what, got, ref):
    """got (bf16) against the float64 ref rounded to bf16: at most one bf16 ulp apart, element by element."""
    got = got.detach().float().cpu().double()
    want = ref.detach().double().cpu().float().to(torch.bfloat16).double()
    big = torch.maximum(got.abs(), want.abs()).clamp_min(2.0 ** -120)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    worst = float(((got - want).abs() / ulp).max())
    print(f"{what}: worst distance {worst:.2f} bf16 ulp")
    assert worst <= 1.0, (what, worst)
    return worst


# ------------------------------------------------------------------------------------------------ the problems
def np_targets(labels, p, C, on, off, row0, rows, binarize=False):
    """mixup_target for the batch rows row0 .. row0 + rows - 1 as the kernels define it: f32 [rows, C] with timm's three roundings
    (y1 lam, y2 (1 - lam), their sum); a partner outside [0, B) or a lam outside [0, 1) means "not mixed"; a label outside
    [0, C) is an all-`off` one-hot row."""
    B = len(labels)
    on, off = np.float32(on), np.float32(off)
    out = np.empty((rows, C), np.float32)
    cols = np.arange(C)
    for r in range(rows):
        i = row0 + r
        partner, lam = int(p.partner[i]), np.float32(p.lam[i])
        if partner < 0 or partner >= B or not (lam >= 0 and lam < 1):
            partner, lam = i, np.float32(1)
        y1 = np.where(cols == labels[i], on, off).astype(np.float32)
        y2 = np.where(cols == labels[partner], on, off).astype(np.float32)
        out[r] = y1 * lam + y2 * (np.float32(1) - lam)
    return (out > 0).astype(np.float32) if binarize else out


@functools.lru_cache(maxsize=None)
def _draw(rows, C, seed=0):
    """A batch of B = rows + 4 samples of which the rows 2 .. rows + 1 are launched (row0 = 2): partners three samples further
    on, so some lie outside the launched rows; by launched row in turn: an ordinary mixed row, a label outside [0, C), a row that
    is "not mixed" (partner -1 or lam 1.5 in turn), a lam near 0; sample 0 - a partner of a launched row - has the label -1."""
    rng = np.random.RandomState(1000 * rows + C + seed)
    B, row0 = rows + 4, 2
    labels = rng.randint(0, C, B).astype(np.int64)
    partner = (np.arange(B) + 3) % B
    lam = rng.uniform(0.05, 0.95, B).astype(np.float32)
    labels[0] = -1
    for r in range(rows):
        i = row0 + r
        if r % 4 == 1:
            labels[i] = C if r % 8 == 1 else -3
        elif r % 4 == 2:
            if r % 8 == 2:
                partner[i] = -1
            else:
                lam[i] = 1.5
        elif r % 4 == 3:
            lam[i] = 1e-6
    p = MixParams(partner, lam, np.zeros(B, bool), np.zeros((B, 4)))
    return labels, p, row0


def _logits(rows, C, dtype, ld, seed, scale=3.0):
    """[rows, C] logits as a column slice of a [rows, ld] buffer whose padding is NaN: a read past a row's C columns shows."""
    rng = np.random.RandomState(seed)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :C] = torch.from_numpy((scale * rng.randn(rows, C)).astype(np.float32))
    return buf.to(dtype).to(DEV)


def _run(fn, leaf, C):
    """loss and the gradient in the first C columns of a leaf that keeps its row stride."""
    x = leaf.detach().clone().requires_grad_(True)
    loss = fn(x[:, :C])
    loss.backward()
    return loss.detach(), x.grad[:, :C]


def _soft_ce(x, t):
    return torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean()


WORST = {}


def _note(key, err, stock):
    ratio = err / stock if stock > 0 else float("inf") if err > 0 else 0.0
    if ratio > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (ratio, err, stock)


# ------------------------------------------------------------------------------------------------ mix_ce: value and gradient
ROWS = [1, 2, 7, 64]
CLASSES = [2, 5, 63, 64, 65, 255, 256, 257, 1000, 1001, 2048, 2049, 21841, 24576, 24577, 50000]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", CLASSES)
@pytest.mark.parametrize("rows", ROWS)
def test_mix_ce_value_and_gradient(rows, C, dtype):
    labels, p, row0 = _draw(rows, C)
    on, off = smoothing_on_off(0.1, C)
    y, table = torch.from_numpy(labels).to(DEV), torch.from_numpy(p.table()).to(DEV)
    t32 = np_targets(labels, p, C, on, off, row0, rows)
    t_dev = torch.from_numpy(t32).to(DEV)
    assert torch.equal(mix_targets(y, table, C, on=on, off=off, binarize=False, row0=row0, rows=rows), t_dev)
    kern = lambda x: mix_ce_loss(x, y, table, on=on, off=off, row0=row0)
    tag = f"mix_ce {'bf16' if dtype == torch.bfloat16 else 'f32'} {rows}x{C}"
    seen = {}
    for ld in (C, C + 3):                                # contiguous and strided: 16-byte accesses where ld allows them
        leaf = _logits(rows, C, dtype, ld, seed=rows + C)
        got_l, got_g = _run(kern, leaf, C)
        assert got_l.dtype == torch.float32 and got_g.dtype == dtype and got_g.shape == (rows, C)
        if ld == C:
            stock_l, stock_g = _run(lambda x: _soft_ce(x.float(), t_dev), leaf, C)
            ref_l, ref_g = _run(lambda x: F.cross_entropy(x, torch.from_numpy(t32).double()), leaf[:, :C].double().cpu(), C)
        _note("ce value", *within(f"{tag} ld {ld} value", got_l.view(1), stock_l.view(1), ref_l.view(1)))
        if dtype == torch.float32:
            _note("ce dlogits f32", *within(f"{tag} ld {ld} dlogits", got_g, stock_g, ref_g))
        else:
            bf16_close(f"{tag} ld {ld} dlogits", got_g, ref_g)
        l2, g2 = _run(kern, leaf, C)                      # two identical launches: bit for bit
        assert torch.equal(l2, got_l) and torch.equal(g2, got_g)
        seen[ld] = (got_l, got_g)
    # the loss and the gradient do not depend on the row stride (one summation order for both access widths)
    assert torch.equal(seen[C][0], seen[C + 3][0]) and torch.equal(seen[C][1], seen[C + 3][1])
    # the halves of the launch on their own: 1 / rows is the only difference, an exact power of two
    if rows % 2 == 0:
        h = rows // 2
        leaf = _logits(rows, C, dtype, C, seed=rows + C)
        for k in (0, 1):
            _, gh = _run(lambda x: mix_ce_loss(x, y, table, on=on, off=off, row0=row0 + k * h), leaf[k * h:(k + 1) * h], C)
            assert torch.equal(gh, seen[C][1][k * h:(k + 1) * h] * 2), k
    # an upstream gradient scales dlogits on the device
    _, gq = _run(lambda x: kern(x) * 0.25, _logits(rows, C, dtype, C, seed=rows + C), C)
    assert torch.equal(gq, seen[C][1] * 0.25)


def test_mix_ce_worst_ratios_are_reported():
    """Not a check of its own: prints the worst kernel / stock error ratios the cases above measured (NOTES quotes them)."""
    for key, (ratio, err, stock) in sorted(WORST.items()):
        print(f"worst {key}: kernel / stock = {ratio:.3f} (kernel {err:.3e}, stock {stock:.3e})")


# ------------------------------------------------------------------------------------------------ mix_ce: extremes
def _identity_problem(rows, C, seed):
    rng = np.random.RandomState(seed)
    labels = rng.randint(0, C, rows).astype(np.int64)
    p = MixParams.identity(rows)
    return labels, p, torch.from_numpy(labels).to(DEV), torch.from_numpy(p.table()).to(DEV)


@pytest.mark.parametrize("C", [1000, 3000])
def test_mix_ce_f32_logits_of_1e4(C):
    rows = 4
    labels, p, y, table = _identity_problem(rows, C, 5)
    on, off = smoothing_on_off(0.1, C)
    rng = np.random.RandomState(6)
    leaf = torch.from_numpy(np.where(rng.rand(rows, C) < 0.5, -1e4, 1e4).astype(np.float32)).to(DEV)
    t32 = np_targets(labels, p, C, on, off, 0, rows)
    got_l, got_g = _run(lambda x: mix_ce_loss(x, y, table, on=on, off=off), leaf, C)
    stock_l, stock_g = _run(lambda x: _soft_ce(x, torch.from_numpy(t32).to(DEV)), leaf, C)
    ref_l, ref_g = _run(lambda x: F.cross_entropy(x, torch.from_numpy(t32).double()), leaf.double().cpu(), C)
    assert bool(torch.isfinite(got_l)) and bool(torch.isfinite(got_g).all()) and bool(torch.isfinite(ref_l))
    within(f"mix_ce f32 +-1e4 C {C} value", got_l.view(1), stock_l.view(1), ref_l.view(1))
    within(f"mix_ce f32 +-1e4 C {C} dlogits", got_g, stock_g, ref_g)


@pytest.mark.parametrize("C", [1000, 3000])
def test_mix_ce_bf16_logits_at_the_largest_bf16(C):
    rows = 4
    labels, p, y, table = _identity_problem(rows, C, 7)
    on, off = smoothing_on_off(0.1, C)
    x = torch.from_numpy((3 * np.random.RandomState(8).randn(rows, C)).astype(np.float32))
    other = [(int(l) + 5) % C for l in labels]
    x[0, labels[0]] = BF16_MAX                           # the label holds the maximum: only the smoothed classes cost
    x[1, other[1]] = -BF16_MAX                           # a smoothed class far below: off (lse - x) is large, finite
    x[2, other[2]] = BF16_MAX                            # another class holds the maximum: the row's loss is ~ on * max
    x[3, other[3]], x[3, (other[3] + 1) % C] = BF16_MAX, -BF16_MAX
    leaf = x.to(torch.bfloat16).to(DEV)
    assert float(leaf.float().abs().max()) == BF16_MAX
    t32 = np_targets(labels, p, C, on, off, 0, rows)
    got_l, got_g = _run(lambda x: mix_ce_loss(x, y, table, on=on, off=off), leaf, C)
    stock_l, _ = _run(lambda x: _soft_ce(x.float(), torch.from_numpy(t32).to(DEV)), leaf, C)
    ref_l, ref_g = _run(lambda x: F.cross_entropy(x, torch.from_numpy(t32).double()), leaf.double().cpu(), C)
    assert bool(torch.isfinite(ref_l)) and float(ref_l) < 3e38
    assert bool(torch.isfinite(got_l)) and bool(torch.isfinite(got_g.float()).all())
    within(f"mix_ce bf16 max C {C} value", got_l.view(1), stock_l.view(1), ref_l.view(1))
    bf16_close(f"mix_ce bf16 max C {C} dlogits", got_g, ref_g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C,ld", [(1000, 1000), (1001, 1004), (2049, 2049), (25000, 25000)])
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_mix_ce_non_finite_logits_stay_inside_the_row(bad, C, ld, dtype):
    """An inf in a row makes the launch's loss non-finite, and neither the logits' nor the gradient's surroundings are touched:
    both live inside larger buffers filled with a sentinel."""
    rows, guard = 3, 2
    labels, p, y, table = _identity_problem(rows, C, 9)
    on, off = smoothing_on_off(0.1, C)
    sentinel = 12345.0
    xbuf = torch.full((rows + 2 * guard, ld + 16), sentinel, dtype=dtype, device=DEV)
    dbuf = torch.full((rows + 2 * guard, ld + 16), sentinel, dtype=dtype, device=DEV)
    x = xbuf[guard:guard + rows, 8:8 + C]                # row stride ld + 16, the rows start 8 elements into the buffer's
    d = dbuf[guard:guard + rows, 8:8 + C]                # (ld 1000 and 25000: 16-byte accesses; 1004: f32 only; 2049: none)
    x.copy_(torch.from_numpy((3 * np.random.RandomState(C).randn(rows, C)).astype(np.float32)).to(dtype))
    x[1, C - 1] = bad
    kept = xbuf.clone()
    loss = torch.zeros((), device=DEV)
    ws = torch.empty(rows, dtype=torch.float64, device=DEV)
    ops.mix_ce(x, y, table, on, off, loss=loss, workspace=ws, dlogits=d)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(loss)), float(loss)
    assert torch.equal(xbuf.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       kept.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    outside = torch.ones_like(dbuf, dtype=torch.bool)
    outside[guard:guard + rows, 8:8 + C] = False
    assert bool((dbuf[outside] == sentinel).all())
    # the rows without the bad logit have their ordinary gradients
    clean = torch.empty(rows, C, dtype=dtype, device=DEV)
    good = x.clone()
    good[1, C - 1] = 0.0
    ops.mix_ce(good, y, table, on, off, dlogits=clean)
    assert torch.equal(d[0], clean[0]) and torch.equal(d[2], clean[2])
    assert bool(torch.isfinite(clean.float()).all())


# ------------------------------------------------------------------------------------------------ mix_ce: equivalences
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("C", [10, 1000])
@pytest.mark.parametrize("s", [0.0, 0.1])
def test_mix_ce_with_the_identity_table_is_cross_entropy(s, C, dtype):
    rows = 8
    labels, p, y, table = _identity_problem(rows, C, 11)
    on, off = smoothing_on_off(s, C)
    assert (on, off) == (1.0, 0.0) or s > 0
    leaf = _logits(rows, C, dtype, C, seed=C)
    got_l, got_g = _run(lambda x: mix_ce_loss(x, y, table, on=on, off=off), leaf, C)
    stock_l, stock_g = _run(lambda x: F.cross_entropy(x.float(), y, label_smoothing=s), leaf, C)
    ref_l, ref_g = _run(lambda x: F.cross_entropy(x, torch.from_numpy(labels), label_smoothing=s), leaf.double().cpu(), C)
    tag = f"mix_ce identity s {s} C {C} {'bf16' if dtype == torch.bfloat16 else 'f32'}"
    within(f"{tag} value", got_l.view(1), stock_l.view(1), ref_l.view(1))
    if dtype == torch.float32:
        within(f"{tag} dlogits", got_g, stock_g, ref_g)
    else:
        bf16_close(f"{tag} dlogits", got_g, ref_g)


def test_mix_ce_refuses_bad_arguments():
    y = torch.zeros(4, dtype=torch.int64, device=DEV)
    table = torch.from_numpy(MixParams.identity(4).table()).to(DEV)
    with pytest.raises(RuntimeError, match="shape"):
        mix_ce_loss(torch.zeros(4, 1, device=DEV), y, table)              # C < 2
    with pytest.raises(RuntimeError, match="shape"):
        mix_ce_loss(torch.zeros(3, 10, device=DEV), y, table, row0=2)      # row0 + rows > B
    with pytest.raises(ValueError):
        mix_ce_loss(torch.zeros(4, 10, device=DEV), y, table[:2])
    with pytest.raises(ValueError):
        cosub_bce_loss(torch.zeros(5, 10, device=DEV), y, table, 1.0, 0.0, True)


# ------------------------------------------------------------------------------------------------ cosub
def _cosub_expr(logits, t):
    bce = F.binary_cross_entropy_with_logits
    a, b = logits.chunk(2)
    return 0.25 * (bce(a, t) + bce(b, t) + bce(a, b.detach().sigmoid()) + bce(b, a.detach().sigmoid()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("binarize", [True, False])
@pytest.mark.parametrize("C", [2, 65, 1000, 1001])
@pytest.mark.parametrize("rows", [1, 3, 32])
def test_cosub_bce_value_and_gradient(rows, C, binarize, dtype):
    labels, p, row0 = _draw(rows, C, seed=1)
    on, off = (1.0, 0.0) if binarize else smoothing_on_off(0.1, C)
    y, table = torch.from_numpy(labels).to(DEV), torch.from_numpy(p.table()).to(DEV)
    t32 = np_targets(labels, p, C, on, off, row0, rows, binarize)
    t_dev = torch.from_numpy(t32).to(DEV)
    assert torch.equal(mix_targets(y, table, C, on=on, off=off, binarize=binarize, row0=row0, rows=rows), t_dev)
    kern = lambda x: cosub_bce_loss(x, y, table, on, off, binarize, row0=row0)
    tag = f"cosub {'bf16' if dtype == torch.bfloat16 else 'f32'} {rows}x{C} {'binarised' if binarize else 'soft'}"
    seen = {}
    for ld in (C, C + 3):
        leaf = _logits(2 * rows, C, dtype, ld, seed=3 * rows + C)
        got_l, got_g = _run(kern, leaf, C)
        assert got_l.dtype == torch.float32 and got_g.dtype == dtype and got_g.shape == (2 * rows, C)
        if ld == C:
            stock_l, stock_g = _run(lambda x: _cosub_expr(x.float(), t_dev), leaf, C)
            ref_l, ref_g = _run(lambda x: _cosub_expr(x, torch.from_numpy(t32).double()), leaf[:, :C].double().cpu(), C)
        within(f"{tag} ld {ld} value", got_l.view(1), stock_l.view(1), ref_l.view(1))
        for half, sl in (("a", slice(0, rows)), ("b", slice(rows, 2 * rows))):
            if dtype == torch.float32:
                within(f"{tag} ld {ld} d{half}", got_g[sl], stock_g[sl], ref_g[sl])
            else:
                bf16_close(f"{tag} ld {ld} d{half}", got_g[sl], ref_g[sl])
        l2, g2 = _run(kern, leaf, C)
        assert torch.equal(l2, got_l) and torch.equal(g2, got_g)
        seen[ld] = (got_l, got_g, leaf)
    assert torch.equal(seen[C][0], seen[C + 3][0]) and torch.equal(seen[C][1], seen[C + 3][1])
    # the symmetric check: swapping the halves swaps the gradients and keeps the loss, bit for bit
    got_l, got_g, leaf = seen[C]
    sw_l, sw_g = _run(kern, torch.cat((leaf[rows:], leaf[:rows])), C)
    assert torch.equal(sw_l, got_l)
    assert torch.equal(sw_g[:rows], got_g[rows:]) and torch.equal(sw_g[rows:], got_g[:rows])
    _, gq = _run(lambda x: kern(x) * 0.5, leaf, C)
    assert torch.equal(gq, got_g * 0.5)


# ------------------------------------------------------------------------------------------------ the trainer
KW = dict(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=64, depth=2, num_heads=2,
          mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=1)
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=10)
CONFIGS = {
    "ce_mixup": dict(loss="ce", mix=True),
    "ce_labels": dict(loss="ce", mix=False, smoothing=0.0),
    "ce_labels_smoothed": dict(loss="ce", mix=False, smoothing=0.1),
    "cosub_bce": dict(loss="bce", mix=True, cosub=True),
    "cosub_ce": dict(loss="ce", mix=True, cosub=True),
}


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _model():
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(0)
    return OcticVisionTransformer(**KW).cuda()


def _batches(n, B=8, seed=100):
    g = _gen(seed)
    return [(torch.randn(B, 3, 32, 32, generator=g, device=DEV), torch.randint(0, 10, (B,), generator=g, device=DEV))
            for _ in range(n)]


def _trainer(name, fused=True, seed=7, **kw):
    from octic_vits_amd.train import Trainer
    cfg = dict(CONFIGS[name])
    mix = Mixup(rng=np.random.RandomState(seed), **MIX) if cfg.pop("mix") else None
    return Trainer(_model(), lr=1e-3, mixup=mix, fused_loss=fused, **cfg, **kw)


def _float64_loss_arm(tr):
    """The unfused trainer with its loss taken in float64 on the same logits: the reference arm of the three-way comparison."""
    from octic_vits_amd import train as T

    def loss64(outputs, targets):
        if tr.cosub:
            return T._cosub_stock(outputs.double(), targets.double())
        return T._soft_target_ce(outputs.double(), targets.double())

    tr._loss = loss64
    return tr


def _flat(tr):
    return torch.cat([p.detach().double().reshape(-1) for p in tr.raw_model.parameters()])


def _same_weights(ta, tb):
    for (n, pa), pb in zip(ta.raw_model.named_parameters(), tb.raw_model.parameters()):
        assert torch.equal(pa, pb), n
    for ea, eb in zip(ta.optimizer.ema_state(), tb.optimizer.ema_state()):
        assert torch.equal(ea, eb)


def _three_arms(name, steps=2, **kw):
    """`steps` steps of the fused trainer, the unfused one and the unfused one with a float64 loss from the same seeds: the fused
    losses and parameters are within the `within` rule of the float64 arm, measured by the unfused (stock f32) arm."""
    fused, stock, ref = _trainer(name, True, **kw), _trainer(name, False, **kw), _float64_loss_arm(_trainer(name, False, **kw))
    losses = {id(t): [] for t in (fused, stock, ref)}
    for x, y in _batches(steps, seed=300):
        for t in (fused, stock, ref):
            losses[id(t)].append(t.step(x, y).double().view(1))
    cat = lambda t: torch.cat(losses[id(t)])
    assert len(set(float(v) for v in cat(fused))) == steps
    within(f"trainer {name} {kw} losses", cat(fused), cat(stock), cat(ref), floor_ulps=1)
    within(f"trainer {name} {kw} parameters", _flat(fused), _flat(stock), _flat(ref), floor_ulps=1)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trainer_fused_agrees_with_unfused(name):
    """The tolerance is the one of tests/test_mixup_gpu.py's fused-against-materialised test (`within`: twice the stock f32 arm's
    error against float64 plus ONE f32 ulp), over two steps and every parameter."""
    _three_arms(name)


def test_trainer_ce_with_accumulation_agrees_with_unfused():
    _three_arms("ce_mixup", accum_steps=2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_trainer_captured_step_equals_eager(name):
    ta, tb = _trainer(name, seed=11), _trainer(name, seed=11)
    batches = _batches(4, seed=200)
    gs = tb.capture(*batches[0], warmup=2)
    for _ in range(2):
        ta.step(*batches[0])
    lb = [gs.replay(x, y).clone() for x, y in batches[1:]]
    la = [ta.step(x, y) for x, y in batches[1:]]
    la, lb = [float(v) for v in la], [float(v) for v in lb]
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)


def test_trainer_ce_dense_targets_take_the_stock_composition():
    from octic_vits_amd.train import Trainer
    x, y = _batches(1, seed=400)[0]
    t = F.one_hot(y, 10).float() * 0.9 + 0.01
    seen = {}
    tr = Trainer(_model(), lr=1e-3, loss="ce")
    hook = tr.raw_model.head.register_forward_hook(lambda m, i, o: seen.__setitem__("logits", o.detach().clone()))
    loss = tr.step(x, t)
    hook.remove()
    assert torch.equal(loss, _soft_ce(seen["logits"].float(), t))


def test_trainer_defaults_run_the_parent_commits_path():
    """Trainer(model, mixup=mix) with the new arguments at their defaults: the same bits as a step written out by hand with
    mix_images and mix_bce_loss (what the trainer ran before it had a `loss` argument)."""
    from octic_vits_amd.train import Trainer
    kw = dict(MIX, label_smoothing=0.0)                  # (the recipe's: with smoothing every binarised target is 1)
    ta = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(5), **kw))
    tb = Trainer(_model(), lr=1e-3)
    mix = Mixup(rng=np.random.RandomState(5), **kw)
    on, off = mix.on_off()
    for x, y in _batches(2, seed=500):
        la = ta.step(x, y)
        table = torch.from_numpy(mix.draw(8, 32, 32).table()).to(DEV)
        tb.model.train()
        tb.optimizer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = tb.model(mix_images(x, table))
            lb = mix_bce_loss(out, y, table, on=on, off=off, binarize=True)
        with tb._batched_finishes():
            lb.backward()
        tb.optimizer.step()
        assert torch.equal(la, lb.detach())
    _same_weights(ta, tb)
