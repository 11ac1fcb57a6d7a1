"""CPU-only: the host side of the criterion selection (octic_mix_ce, octic_cosub_bce, mixup.smoothing_on_off and the Trainer's
loss / smoothing / cosub arguments) - refused arguments before any launch, the formula of the smoothing values, the oracle the
GPU tests of tests/test_criterion_gpu.py lean on (soft-target cross entropy on identity-table targets IS the label-smoothing
cross entropy, in float64), and the Trainer's refusals at construction."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from octic_vits_amd import _lib
from octic_vits_amd.mixup import Mixup, MixParams, cosub_bce_loss, mix_ce_loss, smoothing_on_off

ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4


def _caller(name, with_binarize):
    L = _lib.lib()
    src, dst, tab, lab, out, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
    order = [("logits", out), ("dtype", _lib.F32), ("ldl", 10), ("labels", lab), ("table", tab), ("B", 4), ("row0", 0), ("rows", 2),
             ("nc", 10), ("on", 1.0), ("off", 0.0)] + ([("binarize", 1)] if with_binarize else []) + \
            [("loss", src), ("gscale", None), ("dlogits", dst), ("ldd", 10), ("ws", ws), ("stream", None)]
    return lambda **k: getattr(L, name)(*[k.get(n, v) for n, v in order])


@pytest.mark.parametrize("name,with_binarize", [("octic_mix_ce", False), ("octic_cosub_bce", True)])
def test_abi_argument_validation_without_gpu(name, with_binarize):
    """Rejected arguments return the documented negative codes before any launch; the ABI version did not move."""
    assert _lib.lib().octic_abi_version() == _lib.ABI_VERSION == 20
    call = _caller(name, with_binarize)
    assert call(rows=0) == ESHAPE and call(rows=-1) == ESHAPE
    assert call(nc=1, ldl=1, ldd=1) == ESHAPE and call(nc=0) == ESHAPE
    assert call(ldl=9) == ESHAPE and call(ldd=9) == ESHAPE
    assert call(loss=None, dlogits=None) == ENULL
    assert call(labels=None) == ENULL and call(table=None) == ENULL and call(logits=None) == ENULL
    assert call(ws=None) == ENULL                                        # a loss without its workspace
    assert call(ws=(6 << 20) + 4) == EALIGN                              # the workspace holds doubles
    assert call(row0=3) == ESHAPE and call(row0=2, rows=3) == ESHAPE     # row0 + rows > B
    assert call(row0=-1) == ESHAPE and call(B=0) == ESHAPE
    assert call(dtype=7) == EDTYPE
    assert call(logits=(5 << 20) + 2) == EALIGN and call(labels=(4 << 20) + 4) == EALIGN
    assert call(dtype=_lib.BF16, logits=(5 << 20) + 1) == EALIGN


def test_smoothing_on_off_is_timms_formula():
    for s, C in ((0.0, 1000), (0.1, 1000), (0.1, 21841), (0.3, 2), (0.9, 5)):
        on, off = smoothing_on_off(s, C)
        assert off == s / C and on == 1. - s + s / C
        assert (on, off) == Mixup(label_smoothing=s, num_classes=C).on_off()
    assert smoothing_on_off(0.0, 10) == (1.0, 0.0)


def _identity_targets(y, C, on, off):
    """mixup_target for the identity table (lam = 1, partner = the row itself) in float64: lam onehot + (1 - lam) onehot."""
    p = MixParams.identity(len(y))
    lam = p.lam.astype(np.float64)[:, None]
    oh = lambda lab: np.where(np.arange(C)[None, :] == lab[:, None], on, off)
    return oh(y) * lam + oh(y[p.partner]) * (1. - lam)


@pytest.mark.parametrize("C", [2, 5, 1000])
@pytest.mark.parametrize("s", [0.0, 0.1])
def test_soft_target_ce_on_identity_targets_is_label_smoothing_ce(s, C):
    rng = np.random.RandomState(C)
    x = torch.from_numpy(3 * rng.randn(6, C))
    y = rng.randint(0, C, 6)
    t = torch.from_numpy(_identity_targets(y, C, *smoothing_on_off(s, C)))
    assert t.dtype == x.dtype == torch.float64
    soft = F.cross_entropy(x, t)
    want = F.cross_entropy(x, torch.from_numpy(y), label_smoothing=s)
    assert float((soft - want).abs()) <= 1e-13 * max(1.0, float(want.abs())), (float(soft), float(want))
    # ... and it is the composition the trainer documents for dense targets
    comp = torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean()
    assert float((comp - want).abs()) <= 1e-13 * max(1.0, float(want.abs()))


def test_cpu_tensors_are_refused():
    y = torch.zeros(2, dtype=torch.int64)
    tab = torch.from_numpy(MixParams.identity(2).table())
    with pytest.raises(RuntimeError, match="GPU only"):
        mix_ce_loss(torch.zeros(2, 10), y, tab)
    with pytest.raises(RuntimeError, match="GPU only"):
        cosub_bce_loss(torch.zeros(4, 10), y, tab, 1.0, 0.0, True)


def _net():
    from octic_vits_amd.model import OcticVisionTransformer
    return OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=64, depth=2, num_heads=2,
                                  mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=1)


CPU = dict(fused_optimizer=False, tuned_gemms=False)


def test_trainer_construction_refusals():
    from octic_vits_amd.train import Trainer
    net, mix = _net(), Mixup(num_classes=10)
    with pytest.raises(ValueError, match="loss must be"):
        Trainer(net, loss="nll", **CPU)
    for s in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match="smoothing"):
            Trainer(net, loss="ce", smoothing=s, **CPU)
    with pytest.raises(ValueError, match="needs mixup"):
        Trainer(net, cosub=True, **CPU)
    with pytest.raises(ValueError, match="separate the two passes"):
        Trainer(net, cosub=True, mixup=mix, accum_steps=2, **CPU)
    with pytest.raises(ValueError, match="separate the two passes"):
        Trainer(net, cosub=True, mixup=mix, segment_graphs=2, **CPU)
    # what was refused before still is, with the new arguments at their defaults or not
    with pytest.raises(RuntimeError, match="GPU only"):
        Trainer(net, mixup=mix, loss="ce", **CPU)
    with pytest.raises(RuntimeError, match="GPU only"):
        Trainer(net, mixup=mix, cosub=True, **CPU)


def test_trainer_default_is_unchanged_and_ce_takes_dense_targets_on_the_cpu():
    from octic_vits_amd.train import Trainer
    tr = Trainer(_net(), **CPU)
    assert isinstance(tr.criterion, torch.nn.BCEWithLogitsLoss)
    assert (tr.loss, tr.smoothing, tr.cosub, tr.mixup, tr.fused_loss) == ("bce", 0.0, False, None, True)
    # loss="ce" with dense float targets is the stock composition and needs no GPU; int64 labels need the kernel
    ce = Trainer(_net(), loss="ce", smoothing=0.1, autocast=False, **CPU)
    x = torch.randn(4, 10)
    t = torch.softmax(torch.randn(4, 10), -1)
    assert torch.equal(ce._loss(x, t), torch.sum(-t * F.log_softmax(x, dim=-1), dim=-1).mean())
    with pytest.raises(RuntimeError, match="GPU only"):
        ce.step(torch.zeros(4, 3, 32, 32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="int64 class labels"):
        ce.step(torch.zeros(4, 3, 32, 32), torch.zeros(3, dtype=torch.int64))
