"""CPU-only: the host side of octic_vits_amd.mixup - draw parity with the restatement of timm's Mixup
(tests/golden/mixup_case.py), the invariants of a draw, argument validation of the three C entry points and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import mixup_case
from octic_vits_amd import _lib
from octic_vits_amd.mixup import MixParams, Mixup, mix_bce_loss, mix_images, mix_targets

SHAPES = [(8, 32, 32), (2, 7, 30), (64, 224, 224)]
VARIANTS = {
    "both": dict(mixup_alpha=0.8, cutmix_alpha=1.0),
    "mixup_only": dict(mixup_alpha=0.8, cutmix_alpha=0.0),
    "cutmix_only": dict(mixup_alpha=0.0, cutmix_alpha=1.0),
    "minmax": dict(mixup_alpha=0.8, cutmix_alpha=1.0, cutmix_minmax=(0.2, 0.8)),
    "prob_half": dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.5),
    "uncorrected": dict(mixup_alpha=0.8, cutmix_alpha=1.0, correct_lam=False),
}
CASES = [(mode, name) for mode in ("batch", "pair", "elem") for name in VARIANTS] + [("batch", "off")]


def _kwargs(mode, name):
    kw = dict(mixup_alpha=0.0, cutmix_alpha=0.0) if name == "off" else dict(VARIANTS[name])
    return dict(kw, mode=mode, label_smoothing=0.0, num_classes=10)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("mode,name", CASES)
def test_draws_match_the_timm_restatement_variate_for_variate(mode, name):
    kw = _kwargs(mode, name)
    for si, (B, H, W) in enumerate(SHAPES):
        seed = 1000 * si + 17
        ours, ref = Mixup(**kw), mixup_case.RefMixup(**kw)
        np.random.seed(seed)
        got = [ours.draw(B, H, W) for _ in range(50)]
        state_ours = np.random.get_state()
        np.random.seed(seed)
        x = torch.empty(B, 0, H, W)                     # no pixels: the oracle's slice assignments run, the draws are the point
        y = torch.zeros(B, dtype=torch.int64)
        for k in range(50):
            ref(x, y)
            lam, cut, box = mixup_case.normalised(ref.last)
            want = MixParams(np.arange(B - 1, -1, -1), lam, cut, box)
            assert got[k] == want, (mode, name, (B, H, W), k, got[k], want)
        assert _same_state(state_ours, np.random.get_state()), (mode, name, (B, H, W))
        if name == "off":
            assert all(p == MixParams(np.arange(B - 1, -1, -1), np.ones(B), np.zeros(B, bool), np.zeros((B, 4))) for p in got)
        else:
            assert any((p.lam != 1).any() for p in got)


def test_random_state_argument_reproduces_the_module_stream():
    kw = _kwargs("elem", "both")
    np.random.seed(5)
    a = [Mixup(**kw).draw(8, 32, 32) for _ in range(3)]
    m = Mixup(rng=np.random.RandomState(5), **kw)
    before = np.random.get_state()
    b = [m.draw(8, 32, 32) for _ in range(3)]
    assert a[0] == b[0]
    assert _same_state(before, np.random.get_state())   # a private stream leaves the module's alone


@pytest.mark.parametrize("mode", ["batch", "pair", "elem"])
def test_draw_invariants(mode):
    B, H, W = 8, 32, 36
    for name in ("both", "cutmix_only", "minmax", "prob_half"):
        m = Mixup(rng=np.random.RandomState(3), **_kwargs(mode, name))
        seen_cut = False
        for _ in range(40):
            p = m.draw(B, H, W)
            assert p.partner.dtype == np.int32 and p.lam.dtype == np.float32 and p.cut.dtype == bool and p.box.dtype == np.int32
            assert np.array_equal(p.partner, B - 1 - np.arange(B))
            yl, yh, xl, xh = p.box.T
            assert ((0 <= yl) & (yl <= yh) & (yh <= H) & (0 <= xl) & (xl <= xh) & (xh <= W)).all()
            area = (yh - yl).astype(np.int64) * (xh - xl)
            # corrected lam = 1 - area / (H W), rounded to f32 once
            assert np.array_equal(p.lam[p.cut], (1. - area[p.cut] / float(H * W)).astype(np.float32))
            same = p.lam == 1
            assert not p.cut[same].any() and not p.box[same].any()
            assert not p.box[~p.cut].any()
            if mode == "pair":
                assert np.array_equal(p.lam, p.lam[::-1]) and np.array_equal(p.box, p.box[::-1])
                assert np.array_equal(p.cut, p.cut[::-1])
            if mode == "batch":
                assert (p.lam == p.lam[0]).all() and (p.box == p.box[0]).all()
            seen_cut |= bool(p.cut.any())
        assert seen_cut
    t = p.table()
    assert t.dtype == np.int32 and t.shape == (B, 8)
    assert np.array_equal(t[:, 0], p.partner) and np.array_equal(t[:, 1].view(np.float32), p.lam)
    assert np.array_equal(t[:, 2], p.cut) and np.array_equal(t[:, 3:7], p.box) and not t[:, 7].any()


def test_odd_batch_raises_value_error():
    for mode in ("batch", "pair", "elem"):
        with pytest.raises(ValueError, match="even"):
            Mixup(mode=mode).draw(5, 8, 8)
    with pytest.raises(ValueError):
        Mixup(mode="rows")


def test_smoothing_values_are_timms():
    on, off = Mixup(label_smoothing=0.1, num_classes=1000).on_off()
    assert off == 0.1 / 1000 and on == 1. - 0.1 + 0.1 / 1000
    assert Mixup(label_smoothing=0.0).on_off() == (1.0, 0.0)


def test_abi_argument_validation_without_gpu():
    """Rejected arguments return the documented negative codes before any launch; the ABI version did not move."""
    L = _lib.lib()
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    src, dst, tab, lab, out, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20
    ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4
    # images
    assert L.octic_mix_images(None, dst, tab, 2, 3, 8, 8, None) == ENULL
    assert L.octic_mix_images(src, None, tab, 2, 3, 8, 8, None) == ENULL
    assert L.octic_mix_images(src, dst, None, 2, 3, 8, 8, None) == ENULL
    assert L.octic_mix_images(src, dst, tab, 0, 3, 8, 8, None) == ESHAPE
    assert L.octic_mix_images(src, dst, tab, -2, 3, 8, 8, None) == ESHAPE
    assert L.octic_mix_images(src, dst, tab, 2, 3, 0, 8, None) == ESHAPE
    assert L.octic_mix_images(src, dst, tab, 2, 1 << 15, 1 << 8, 1 << 8, None) == ESHAPE     # C H W >= 2^31
    assert L.octic_mix_images(src, src + 2, tab, 2, 3, 8, 8, None) == EALIGN
    nbytes = 2 * 3 * 8 * 8 * 4
    for d in (src, src + 16, src + nbytes - 4, src - nbytes + 4):                            # overlapping src / dst
        assert L.octic_mix_images(src, d, tab, 2, 3, 8, 8, None) == ESHAPE
    # targets
    assert L.octic_mix_targets(None, tab, 2, 0, 2, 10, 1.0, 0.0, 0, out, None) == ENULL
    assert L.octic_mix_targets(lab, None, 2, 0, 2, 10, 1.0, 0.0, 0, out, None) == ENULL
    assert L.octic_mix_targets(lab, tab, 2, 0, 2, 10, 1.0, 0.0, 0, None, None) == ENULL
    assert L.octic_mix_targets(lab, tab, 0, 0, 2, 10, 1.0, 0.0, 0, out, None) == ESHAPE
    assert L.octic_mix_targets(lab, tab, 2, 0, 2, 0, 1.0, 0.0, 0, out, None) == ESHAPE
    assert L.octic_mix_targets(lab, tab, 2, 1, 2, 10, 1.0, 0.0, 0, out, None) == ESHAPE      # row0 + rows > B
    assert L.octic_mix_targets(lab, tab, 2, -1, 2, 10, 1.0, 0.0, 0, out, None) == ESHAPE
    assert L.octic_mix_targets(lab + 4, tab, 2, 0, 2, 10, 1.0, 0.0, 0, out, None) == EALIGN
    # loss
    bce = lambda **k: L.octic_mix_bce(*[k.get(n, v) for n, v in (
        ("logits", out), ("dtype", _lib.F32), ("ldl", 10), ("labels", lab), ("table", tab), ("B", 2), ("row0", 0), ("rows", 2),
        ("nc", 10), ("on", 1.0), ("off", 0.0), ("binarize", 1), ("loss", src), ("gscale", None), ("dlogits", dst), ("ldd", 10),
        ("ws", ws), ("stream", None))])
    assert bce(logits=None) == ENULL and bce(labels=None) == ENULL and bce(table=None) == ENULL
    assert bce(loss=None, dlogits=None) == ENULL and bce(ws=None) == ENULL
    assert bce(B=0) == ESHAPE and bce(nc=0) == ESHAPE and bce(rows=0) == ESHAPE and bce(row0=1) == ESHAPE
    assert bce(ldl=9) == ESHAPE and bce(ldd=9) == ESHAPE
    assert bce(dtype=7) == EDTYPE
    assert bce(logits=out + 2) == EALIGN and bce(ws=ws + 4) == EALIGN


def test_cpu_tensors_are_refused():
    m = Mixup(num_classes=10)
    x, y = torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.int64)
    tab = torch.from_numpy(MixParams.identity(2).table())
    with pytest.raises(RuntimeError, match="GPU only"):
        m.apply(x, y)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(x, y)
    with pytest.raises(RuntimeError, match="GPU only"):
        mix_images(x, tab)
    with pytest.raises(RuntimeError, match="GPU only"):
        mix_targets(y, tab, 10)
    with pytest.raises(RuntimeError, match="GPU only"):
        mix_bce_loss(torch.zeros(2, 10), y, tab)
    from octic_vits_amd.train import evaluate
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluate(torch.nn.Linear(3, 3), [(x, y)])


def test_trainer_with_mixup_refuses_the_cpu_and_float_targets():
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.train import Trainer
    net = OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=2, num_heads=2,
                                 mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=1)
    with pytest.raises(RuntimeError, match="GPU only"):
        Trainer(net, mixup=Mixup(num_classes=10), fused_optimizer=False)
    # the check in front of every step of a mixing trainer: float (already mixed) targets are an error, labels pass
    x = torch.zeros(4, 3, 32, 32)
    with pytest.raises(TypeError, match="int64 class labels"):
        Trainer._mix_check(x, torch.zeros(4, 10))
    with pytest.raises(TypeError, match="int64 class labels"):
        Trainer._mix_check(x, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU only"):
        Trainer._mix_check(x, torch.zeros(4, dtype=torch.int64))
