"""csrc/augment.hip, octic_vits_amd.augment, Trainer(augment=...) and train.evaluate on uint8 batches, on the GPU.

Everything here is bit for bit, no tolerance anywhere: the kernels' uint8 pixels against PIL's recorded results
(tests/golden/augment.npz) and, at sizes the file cannot carry, against the numpy restatement of the contract
(tests/golden/augment_numpy.py, itself held against the golden file and live PIL by tests/test_augment_host.py); the f32 output
against torch's ToTensor + Normalize arithmetic on the CPU; the trainer against a twin fed the augmented f32 batch.  Neither PIL
nor the reference is read here."""
import os
import random

import numpy as np
import pytest
import torch

import augment_numpy
from octic_vits_amd.augment import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, AugParams, ThreeAugment, to_tensor
from octic_vits_amd.mixup import Mixup

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz"))
KEYS = [f"{h}x{w}" for h, w in GOLDEN["shapes"]]
FIELDS = ("flip", "op", "radius", "order", "brightness", "contrast", "saturation")
MEAN, STD = torch.tensor(IMAGENET_DEFAULT_MEAN), torch.tensor(IMAGENET_DEFAULT_STD)


def golden_params(key):
    return AugParams(*[GOLDEN[f"{f}_{key}"] for f in FIELDS])


def row_dict(p, i):
    return dict(flip=bool(p.flip[i]), op=int(p.op[i]), radius=float(p.radius[i]), order=[int(v) for v in p.order[i]],
                brightness=float(p.brightness[i]), contrast=float(p.contrast[i]), saturation=float(p.saturation[i]))


def normalized(u8):
    """ToTensor + Normalize by torch on the CPU: uint8 [B, H, W, 3] -> f32 [B, 3, H, W]."""
    return ((u8.float() / 255 - MEAN) / STD).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("key", KEYS)
def test_kernels_equal_pil_on_every_golden_case(key):
    p = golden_params(key)
    src = torch.from_numpy(GOLDEN["src_" + key]).to(DEV)
    want = torch.from_numpy(GOLDEN["out_" + key])
    kept = src.clone()
    aug = ThreeAugment()
    got = aug.apply(src, p, uint8_out=True)
    assert got.dtype == torch.uint8 and got.shape == src.shape
    bad = [i for i in range(len(p)) if not torch.equal(got[i].cpu(), want[i])]
    assert not bad, (key, [(i, row_dict(p, i)) for i in bad[:3]])
    f = aug.apply(src, p)
    assert f.dtype == torch.float32 and f.shape == (len(p), 3) + tuple(src.shape[1:3])
    assert torch.equal(f.cpu(), normalized(want))
    assert torch.equal(src, kept)                        # the input is left untouched
    # into a caller's buffers, and one sample at a time (another batch size, another grid)
    buf8, buf = torch.zeros_like(src), torch.full_like(f, float("nan"))
    assert aug.apply(src, p, out=buf8, uint8_out=True) is buf8 and torch.equal(buf8, got)
    assert aug.apply(src, p, out=buf) is buf and torch.equal(buf, f)
    i = len(p) // 2
    one = AugParams(*[getattr(p, n)[i:i + 1] for n in FIELDS])
    assert torch.equal(aug.apply(src[i:i + 1].contiguous(), one, uint8_out=True)[0], got[i])


def mixed_params(B, rs):
    """Every op in the batch, every sample with a contrast op somewhere in a full jitter order."""
    orders = [[1, 0, 2, -1], [-1, 2, 0, 1], [0, 1, -1, 2], [2, -1, 1, 0]]
    f = lambda: rs.uniform(0.7, 1.3, B).astype(np.float32)
    return AugParams(flip=np.arange(B) % 2 == 0, op=(3 - np.arange(B)) % 4, radius=rs.choice([0.9, 1.42, 2.0, 0.37], B),
                     order=[orders[(i + B) % 4] for i in range(B)], brightness=f(), contrast=f(), saturation=f())


@pytest.fixture(scope="module")
def large_cases():
    """(src, params, expected uint8) by the numpy restatement, computed once: B = 4 at 224 x 224, B = 2 at 97 x 131 (partial
    tiles, W % 4 != 0), B = 1 at 384 x 384 (more than one CU's LDS could hold), each with mixed ops per sample."""
    rs = np.random.RandomState(11)
    out = {}
    for B, H, W in [(4, 224, 224), (2, 97, 131), (1, 384, 384)]:
        src = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        src[0, : H // 2] //= 3                           # a darker half: the image mean is no mid-grey
        p = mixed_params(B, rs)
        if B == 1:
            p.op[0] = 3                                  # the one large image is blurred
        out[(B, H, W)] = (src, p, np.stack([augment_numpy.apply_u8(src[i], row_dict(p, i)) for i in range(B)]))
    return out


@pytest.mark.parametrize("shape", [(4, 224, 224), (2, 97, 131), (1, 384, 384)])
def test_kernels_equal_the_numpy_restatement_at_large_sizes(large_cases, shape):
    src, p, want = large_cases[shape]
    x = torch.from_numpy(src).to(DEV)
    aug = ThreeAugment()
    got = aug.apply(x, p, uint8_out=True).cpu()
    assert torch.equal(got, torch.from_numpy(want)), [int((got[i] != torch.from_numpy(want[i])).sum()) for i in range(len(p))]
    assert torch.equal(aug.apply(x, p).cpu(), normalized(torch.from_numpy(want)))
    assert torch.equal(x.cpu(), torch.from_numpy(src))


def test_to_tensor_is_the_identity_row_and_other_statistics():
    rs = np.random.RandomState(3)
    src = torch.from_numpy(rs.randint(0, 256, (3, 19, 70, 3)).astype(np.uint8))
    x = src.to(DEV)
    aug = ThreeAugment()
    want = normalized(src)
    assert torch.equal(aug.to_tensor(x).cpu(), want) and torch.equal(to_tensor(x).cpu(), want)
    assert torch.equal(aug.apply(x, AugParams.identity(3)).cpu(), want)
    assert torch.equal(aug.apply(x, AugParams.identity(3), uint8_out=True), x)
    other = ThreeAugment(mean=(0.5, 0.4, 0.3), std=(0.2, 0.25, 0.5))
    ref = ((src.float() / 255 - torch.tensor([0.5, 0.4, 0.3])) / torch.tensor([0.2, 0.25, 0.5])).permute(0, 3, 1, 2)
    assert torch.equal(other.to_tensor(x).cpu(), ref)
    # a fresh draw through __call__: the draw is the host's, the pixels are the restatement's
    aug = ThreeAugment(rng=random.Random(1), generator=torch.Generator().manual_seed(2))
    twin = ThreeAugment(rng=random.Random(1), generator=torch.Generator().manual_seed(2))
    p = twin.draw(3)
    exp = np.stack([augment_numpy.apply_u8(src[i].numpy(), row_dict(p, i)) for i in range(3)])
    assert torch.equal(aug(x).cpu(), normalized(torch.from_numpy(exp)))


def test_unsafe_rows_and_bad_arguments():
    """A table row the kernels cannot trust does nothing harmful: an unknown op or box radius means no op, an unknown or
    repeated jitter entry is skipped.  Wrong tensors are refused before any launch."""
    from octic_vits_amd import ops
    rs = np.random.RandomState(5)
    src = torch.from_numpy(rs.randint(0, 256, (4, 9, 11, 3)).astype(np.uint8)).to(DEV)
    t = AugParams.identity(4).table()
    t[0, 1] = 9
    t[1, 1], t[1, 2] = 3, 5
    t[2, 5:9] = [0, 0, 7, -5]
    t[2, 9] = np.float32(1.25).view(np.int32)
    t[3, 1] = -1
    aug = ThreeAugment()
    got = aug.launch(src, torch.from_numpy(t).to(DEV), uint8_out=True).cpu().numpy()
    s = src.cpu().numpy()
    assert np.array_equal(got[[0, 1, 3]], s[[0, 1, 3]])
    assert np.array_equal(got[2], augment_numpy.blend(0, s[2], 1.25))
    with pytest.raises(ValueError, match="table"):
        aug.launch(src, torch.from_numpy(t[:3].copy()).to(DEV))
    with pytest.raises(ValueError, match="another batch size"):
        aug.apply(src, AugParams.identity(3))
    with pytest.raises(TypeError):
        aug.apply(src, out=torch.empty(4, 3, 9, 11, device=DEV), uint8_out=True)
    with pytest.raises(ValueError, match="output"):
        aug.apply(src, out=torch.empty(4, 3, 11, 9, device=DEV))
    with pytest.raises(ValueError, match="workspace"):
        ops.augment_u8(src, torch.from_numpy(t).to(DEV), aug.mean, aug.std, torch.empty(4, 3, 9, 11, device=DEV),
                       workspace=torch.empty(1, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="shape"):       # the library's own overlap check
        ops.augment_u8(src, torch.from_numpy(t).to(DEV), aug.mean, aug.std, src)


# ------------------------------------------------------------------------------------------------ the trainer
KW = dict(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=4, num_heads=2,
          mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=2)
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=10)


def _model():
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(0)
    return OcticVisionTransformer(**KW).cuda()


def _aug(seed):
    return ThreeAugment(rng=random.Random(seed), generator=torch.Generator().manual_seed(seed + 1))


def _batches(n, B=8, seed=100):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [(torch.randint(0, 256, (B, 32, 32, 3), generator=g, device=DEV, dtype=torch.uint8),
             torch.randint(0, 10, (B,), generator=g, device=DEV)) for _ in range(n)]


def _same_weights(ta, tb):
    for (n, pa), pb in zip(ta.raw_model.named_parameters(), tb.raw_model.parameters()):
        assert torch.equal(pa, pb), n
    for ea, eb in zip(ta.optimizer.ema_state(), tb.optimizer.ema_state()):
        assert torch.equal(ea, eb)


def test_trainer_eager_step_equals_a_twin_fed_the_augmented_batch():
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(7), **MIX), augment=_aug(3))
    tb = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(7), **MIX))
    aug = _aug(3)
    la, lb = [], []
    for x, y in _batches(2):
        la.append(float(ta.step(x, y)))
        lb.append(float(tb.step(aug.apply(x), y)))
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)
    with pytest.raises(TypeError, match=r"uint8 \[B, H, W, 3\]"):
        ta.step(aug.apply(x), y)
    with pytest.raises(RuntimeError, match="GPU only"):
        ta.step(x.cpu(), y)


def test_trainer_without_mixup_takes_uint8_and_float_targets():
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, augment=_aug(9))
    tb = Trainer(_model(), lr=1e-3)
    aug = _aug(9)
    x, y = _batches(1, seed=50)[0]
    t = torch.nn.functional.one_hot(y, 10).float()
    assert float(ta.step(x, t)) == float(tb.step(aug.apply(x), t))
    _same_weights(ta, tb)


@pytest.mark.parametrize("accum", [1, 2])
def test_trainer_captured_step_equals_eager(accum):
    """Eager against captured with the augmentation, the mix and the fused loss inside the graph: three replays with fresh draws,
    issued back to back, nothing read before the end."""
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, accum_steps=accum, mixup=Mixup(rng=np.random.RandomState(11), **MIX), augment=_aug(21))
    tb = Trainer(_model(), lr=1e-3, accum_steps=accum, mixup=Mixup(rng=np.random.RandomState(11), **MIX), augment=_aug(21))
    batches = _batches(4, seed=200 + accum)
    gs = tb.capture(*batches[0], warmup=2)
    assert gs.samples.dtype == torch.uint8               # the graph's input buffer is the uint8 batch
    for _ in range(2):
        ta.step(*batches[0])
    lb = [gs.replay(x, y).clone() for x, y in batches[1:]]
    la = [ta.step(x, y) for x, y in batches[1:]]
    la, lb = [float(v) for v in la], [float(v) for v in lb]
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)


def test_evaluate_takes_uint8_batches():
    from octic_vits_amd.train import evaluate
    net = _model()
    batches = _batches(2, seed=300)
    a = evaluate(net, batches, graphed=False)
    b = evaluate(net, [(to_tensor(x), y) for x, y in batches], graphed=False)
    assert a == b and a["loss"] == a["loss"]
