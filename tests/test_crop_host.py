"""The host side of the DeiT-III crops (octic_vits_amd/crop.py, csrc/crop.hip's declarations), without a GPU: the numpy
restatement against PIL's recorded pixels (tests/golden/crop.npz) and against live PIL where it imports, the draws variate for
variate against hand-written replays of the seeded streams, torchvision's size rules, and the refusals."""
import math
import os
import random

import numpy as np
import pytest
import torch

import crop_numpy as N
from octic_vits_amd import _lib, crop as C, ops
from octic_vits_amd.augment import AugParams, ThreeAugment
from octic_vits_amd.dino_augment import PackedImages, resize_taps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "crop.npz"))


def golden_cases():
    return [(int(r[0]), c) for r, c in zip(GOLDEN["cases"], N.unpack(GOLDEN["cases"][:, 1:]))]


# ------------------------------------------------------------------------------------------------ the contract
def test_the_restatement_equals_pils_recorded_pixels():
    at = {16: 0, 17: 0}
    cases = golden_cases()
    assert len(cases) > 100
    for s, c in cases:
        S = c["out"][0]
        assert np.array_equal(N.apply_u8(GOLDEN[f"src_{s}"], c), GOLDEN[f"out_{S}"][at[S]]), c
        at[S] += 1
    assert all(at[S] == len(GOLDEN[f"out_{S}"]) for S in at)
    # the file covers every mode: the full window, a window inside a non-square resize, reflected corners, all orientations
    assert {(c["rot"], c["flip"]) for _, c in cases} == {(r, f) for r in range(4) for f in (False, True)}
    assert any(c["pad"] and c["win"] == (0, 0) for _, c in cases) and any(c["pad"] and min(c["win"]) > 0 for _, c in cases)
    assert any(c["rsize"][0] != c["rsize"][1] and min(c["win"]) > 0 and not c["pad"] for _, c in cases)
    assert any(c["box"][2] == c["rsize"][0] for _, c in cases) and any(c["box"][3] == c["rsize"][1] for _, c in cases)


def test_the_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    import make_crop_golden as M
    for s, c in golden_cases()[::3]:
        assert np.array_equal(M.pil_apply(GOLDEN[f"src_{s}"], c), N.apply_u8(GOLDEN[f"src_{s}"], c)), c
    rs = np.random.RandomState(3)
    src = rs.randint(0, 256, (45, 61, 3)).astype(np.uint8)
    for S in (15, 16, 17):
        c = C.EvalTransform(size=S, rot=True, flip=True, rng=random.Random(S)).draw([45], [61]).case(0)
        assert np.array_equal(M.pil_apply(src, c), N.apply_u8(src, c)), c
        c = C.SrcCrop(size=S, generator=torch.Generator().manual_seed(S)).draw([45], [61]).case(0)
        assert np.array_equal(M.pil_apply(src, c), N.apply_u8(src, c)), c


def test_symbols_are_declared_exported_documented_and_the_abi_is_20():
    names = ["octic_crop_resize_max_taps", "octic_crop_resize_rows", "octic_crop_resize_u8"]
    declared = _lib.header_symbols()
    L = _lib.lib()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for n in names:
        assert n in declared and n in _lib._PROTOS and hasattr(L, n) and n in text, n
    assert "octic_crop_row" in open(_lib.HEADER_PATH).read()
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    assert ops.CROP_ROW_WORDS == C.ROW_WORDS == 20
    assert ops.crop_resize_rows() >= 1
    assert L.octic_crop_resize_max_taps(4) == -1 and L.octic_crop_resize_max_taps(4097) == -1
    assert [ops.crop_resize_max_taps(S) for S in (5, 16, 224, 4096)] == [49152 // ((3 * S + 3) // 4 * 4) for S in (5, 16, 224, 4096)]
    assert ops.crop_resize_max_taps(224) == resize_taps(4032, 224) == 73   # sources of up to 4032 pixels a side at the recipe's size
    # argument checks in front of any launch
    assert L.octic_crop_resize_u8(None, 1, None, None, 1, 1, 8, 8, None, _lib.U8, 0, 0, 0, 1, 1, 1, None) == -4
    assert L.octic_crop_resize_u8(4096, 64, 8192, 12288, 8, 1, 4, 8, 16384, _lib.U8, 0, 0, 0, 1, 1, 1, None) == -1
    assert L.octic_crop_resize_u8(4096, 64, 8192, 12288, 8, 1, 8, 8, 16384, 99, 0, 0, 0, 1, 1, 1, None) < 0
    assert L.octic_crop_resize_u8(4096, 64, 8196, 12288, 8, 1, 8, 8, 16384, _lib.U8, 0, 0, 0, 1, 1, 1, None) == -2
    assert L.octic_crop_resize_u8(4096, 64, 8192, 12288, 8, 1, 8, 8, 16386, _lib.F32, 0, 0, 0, 1, 1, 1, None) == -2
    assert L.octic_crop_resize_u8(4096, 64, 8192, 12288, 8, 1, 8, 8, 4100, _lib.U8, 0, 0, 0, 1, 1, 1, None) == -1   # dst inside data


# ------------------------------------------------------------------------------------------------ the draws
class Counting(random.Random):
    """A ``random.Random`` that counts the calls the crops make."""

    def __init__(self, seed):
        super().__init__(seed)
        self.calls = []

    def uniform(self, a, b):
        self.calls.append("uniform")
        return super().uniform(a, b)

    def randint(self, a, b):
        self.calls.append("randint")
        return super().randint(a, b)


def replay_rrc(r, H, W, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """timm's get_params written out by hand: ((top, left, h, w), tries, fallback)."""
    for t in range(10):
        area = r.uniform(scale[0], scale[1]) * H * W
        aspect = math.exp(r.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w, h = int(round(math.sqrt(area * aspect))), int(round(math.sqrt(area / aspect)))
        if w <= W and h <= H:
            i = r.randint(0, H - h)
            return (i, r.randint(0, W - w), h, w), t + 1, False
    if W / H < ratio[0]:
        w, h = W, int(round(W / ratio[0]))
    elif W / H > ratio[1]:
        h, w = H, int(round(H * ratio[1]))
    else:
        w, h = W, H
    return ((H - h) // 2, (W - w) // 2, h, w), 10, True


def test_random_resized_crop_consumes_pythons_random_as_timm_does():
    sizes = [(375, 500), (500, 375), (64, 64), (30, 100), (4, 400), (100, 40)]
    tries = 0
    for seed in range(6):
        rng = Counting(seed)
        twin = random.Random(seed)
        crop = C.RandomResizedCrop(size=16, rng=rng)
        for H, W in sizes:
            before = len(rng.calls)
            box = crop.get_params(H, W)
            want, t, fell = replay_rrc(twin, H, W)
            assert box == want, (seed, H, W)
            calls = rng.calls[before:]
            assert calls == ["uniform", "uniform"] * t + ([] if fell else ["randint", "randint"]), (seed, H, W, calls)
            if (H, W) == (4, 400):
                assert fell                                   # every try needs h >= sqrt(0.08 * 1600 * 3 / 4) > 4: the fallback
            if fell:
                assert box == (0, 197, 4, 5)
            tries += t
        assert rng.random() == twin.random()                  # the streams are where the replay left them
    assert tries > 6 * (len(sizes) - 1 + 10)                   # beside the fallback's ten, some tries were refused and drawn again
    p = C.RandomResizedCrop(size=16, rng=random.Random(1)).draw([375, 4], [500, 400])
    assert p.rsize.tolist() == [[16, 16]] * 2 and not p.pad.any() and not p.win.any() and not p.rot.any() and not p.flip.any()
    taller = C.RandomResizedCrop(size=16, rng=random.Random(1)).get_params(400, 4)      # in_ratio below 3/4
    assert taller == (197, 0, 5, 4)


def test_src_crop_draws_nothing_when_the_padded_size_is_the_output():
    g = torch.Generator().manual_seed(4)
    state = g.get_state().clone()
    crop = C.SrcCrop(size=16, padding=0, generator=g)
    p = crop.draw([16, 48], [16, 48])
    assert torch.equal(g.get_state(), state) and p.win.tolist() == [[0, 0], [0, 0]] and p.rsize.tolist() == [[16, 16], [16, 16]]
    # ... and otherwise randint(0, ph - S + 1), then randint(0, pw - S + 1), from the generator it was given
    crop = C.SrcCrop(size=16, padding=4, generator=g)
    twin = torch.Generator().manual_seed(4)
    p = crop.draw([16, 32, 40], [16, 64, 20])
    want = []
    for rh, rw in ((16, 16), (16, 32), (32, 16)):
        want.append([int(torch.randint(0, rh + 8 - 16 + 1, (1,), generator=twin)), int(torch.randint(0, rw + 8 - 16 + 1, (1,), generator=twin))])
    assert p.win.tolist() == want and p.pad.tolist() == [4, 4, 4] and p.rsize.tolist() == [[16, 16], [16, 32], [32, 16]]
    assert torch.equal(g.get_state(), twin.get_state())
    assert p.box.tolist() == [[0, 0, 16, 16], [0, 0, 32, 64], [0, 0, 40, 20]]


def test_resize_int_size_rule():
    assert C.resize_size(500, 375, 256) == (341, 256)          # portrait: int(256 * 500 / 375)
    assert C.resize_size(375, 500, 256) == (256, 341)          # landscape
    assert C.resize_size(300, 300, 224) == (224, 224)          # square
    assert C.resize_size(224, 333, 224) == (224, 333) and C.resize_size(333, 224, 224) == (333, 224)   # short == size: unchanged
    assert C.resize_size(3, 1000, 7) == (7, 2333) and C.resize_size(1, 6, 18) == (18, 108)
    assert C.resize_size(480, 640, 256) == (256, 341) and C.resize_size(333, 500, 256) == (256, 384)   # truncation, not rounding


def test_center_crop_rounds_half_to_even():
    assert [C.center_crop_offset(s, 224) for s in (224, 225, 226, 227, 229, 256, 341)] == [0, 0, 1, 2, 2, 16, 58]
    p = C.EvalTransform().draw([375, 500], [500, 375])         # 341 - 224 = 117: an odd margin, 58.5 -> 58
    assert p.rsize.tolist() == [[256, 341], [341, 256]] and p.win.tolist() == [[16, 58], [58, 16]]
    p = C.make_classification_eval_transform(resize_size=20, crop_size=17).draw([40], [30])
    assert p.rsize.tolist() == [[26, 20]] and p.win.tolist() == [[4, 2]]      # 4.5 -> 4, 1.5 -> 2
    rng, twin = random.Random(8), random.Random(8)
    p = C.EvalTransform(size=16, rot=True, flip=True, rng=rng).draw([20] * 12, [30] * 12)
    assert p.rot.tolist() == [twin.choice([0, 90, 180, 270]) // 90 for _ in range(12)] and len(set(p.rot.tolist())) == 4
    assert p.flip.all() and rng.random() == twin.random()


# ------------------------------------------------------------------------------------------------ 3-Augment's stream order
def _three(seed, crop=None):
    return ThreeAugment(rng=random.Random(seed), generator=torch.Generator().manual_seed(seed + 1), crop=crop)


def test_draw_sources_interleaves_the_crop_and_the_augmentation_per_sample():
    H, W = [375, 64, 4, 200, 90], [500, 48, 400, 30, 90]
    rng = random.Random(12)                                    # ONE stream for the crop and the augmentation, as in the reference
    aug = ThreeAugment(rng=rng, generator=torch.Generator().manual_seed(13), crop=C.RandomResizedCrop(size=16, rng=rng))
    cp, ap = aug.draw_sources(H, W)
    # a replay by hand: per sample the crop's draws, then the augmentation's
    twin_rng = random.Random(12)
    twin = ThreeAugment(rng=twin_rng, generator=torch.Generator().manual_seed(13))
    boxes, want = [], AugParams.identity(5)
    for i in range(5):
        boxes.append(replay_rrc(twin_rng, H[i], W[i])[0])
        one = twin.draw(1)
        for n in ("flip", "op", "radius", "order", "brightness", "contrast", "saturation"):
            getattr(want, n)[i] = getattr(one, n)[0]
    assert cp.box.tolist() == [list(b) for b in boxes] and ap == want
    assert rng.random() == twin_rng.random()
    # not interleaved, the same seeds give other boxes: the order is observable
    flat = random.Random(12)
    assert [replay_rrc(flat, h, w)[0] for h, w in zip(H, W)] != boxes
    # separate streams: the crop rows of a crop-only replay and the AugParams of a replay that skips the crop draws
    aug = _three(20, crop=C.RandomResizedCrop(size=16, rng=random.Random(30)))
    cp, ap = aug.draw_sources(H, W)
    assert cp == C.RandomResizedCrop(size=16, rng=random.Random(30)).draw(H, W)
    assert ap == _three(20).draw(5)
    t = cp.tables()
    assert np.array_equal(t["rows"], C.RandomResizedCrop(size=16, rng=random.Random(30)).draw(H, W).tables()["rows"])
    # --src draws from torch's generator, between the augmentation's own torch draws
    g = torch.Generator().manual_seed(40)
    aug = ThreeAugment(rng=random.Random(41), generator=g, crop=C.SrcCrop(size=16, generator=g))
    cp, ap = aug.draw_sources(H, W)
    g2 = torch.Generator().manual_seed(40)
    twin, src = ThreeAugment(rng=random.Random(41), generator=g2), C.SrcCrop(size=16, generator=g2)
    for i in range(5):
        assert cp.win[i].tolist() == list(src.draw_one(H[i], W[i])["win"])
        assert ap.brightness[i] == twin.draw(1).brightness[0]
    with pytest.raises(RuntimeError, match="without `crop`"):
        _three(1).draw_sources(H, W)
    with pytest.raises(TypeError, match="transform of octic_vits_amd.crop"):
        ThreeAugment(crop=object())


def test_draw_is_bitwise_the_draw_of_the_parent():
    """Recorded from the code in front of this feature: ThreeAugment(rng=Random(5), generator=manual_seed(6)).draw(6)."""
    for crop in (None, C.RandomResizedCrop(rng=random.Random(0))):
        p = ThreeAugment(rng=random.Random(5), generator=torch.Generator().manual_seed(6), crop=crop).draw(6)
        assert p.flip.tolist() == [False, False, True, True, True, False]
        assert p.op.tolist() == [2, 3, 3, 3, 1, 1]
        assert [float(v).hex() for v in p.radius] == ["0x0.0p+0", "0x1.817c96313e57cp+0", "0x1.f8286037f4e11p-1", "0x1.cfcc49acbc8f4p+0",
                                                      "0x0.0p+0", "0x0.0p+0"]
        assert p.order.tolist() == [[1, 0, 2, -1], [0, 1, -1, 2], [2, 1, -1, 0], [0, -1, 2, 1], [1, 0, 2, -1], [-1, 0, 1, 2]]
        assert p.brightness.view(np.int32).tolist() == [1062682175, 1064998400, 1063993997, 1064269388, 1067284433, 1063292163]
        assert p.contrast.view(np.int32).tolist() == [1064841639, 1066023856, 1062872642, 1062210537, 1061273269, 1067595354]
        assert p.saturation.view(np.int32).tolist() == [1066230679, 1066708375, 1061972981, 1067051734, 1066759680, 1065361656]


# ------------------------------------------------------------------------------------------------ tables and refusals
def test_tables_hold_the_rows_the_header_declares():
    p = C.CropParams([40, 30], [50, 60], 16, 16, box=[(1, 2, 30, 40), (0, 0, 30, 60), (5, 5, 16, 16)], source=[0, 1, 0],
                     rsize=[(16, 16), (20, 40), (16, 16)], pad=[0, 4, 0], win=[(0, 0), (12, 32), (0, 0)], rot=[0, 3, 2], flip=[False, True, False])
    t = p.tables()
    rows, coef = t["rows"], t["coef"]
    assert rows.shape == (3, 20) and rows.dtype == np.int32 and coef.dtype == np.int32
    assert rows[:, 0:2].copy().view(np.int64).reshape(-1).tolist() == [0, 40 * 50 * 3, 0]
    assert rows[1, 2:15].tolist() == [30, 60, 0, 0, 30, 60, 20, 40, 4, 12, 32, 3, 1] and not rows[:, 19].any()
    for i, (w, rw, h, rh) in enumerate([(40, 16, 30, 16), (60, 40, 30, 20), (16, 16, 16, 16)]):
        for word, n, r in ((15, w, rw), (17, h, rh)):
            at, taps = int(rows[i, word]), int(rows[i, word + 1])
            bounds, k = ops.dino_resize_coeffs(n, r, resize_taps(n, r))
            assert taps == resize_taps(n, r)
            assert np.array_equal(coef[at:at + 2 * r], bounds.reshape(-1)) and np.array_equal(coef[at + 2 * r:at + 2 * r + r * taps], k.reshape(-1))
    assert rows[2, 15] == rows[2, 17]                          # one block per distinct (length, resized length)
    assert p.case(1) == dict(box=(0, 0, 30, 60), rsize=(20, 40), pad=4, win=(12, 32), out=(16, 16), rot=3, flip=True)


def test_refusals():
    cpu = PackedImages(torch.zeros(40 * 50 * 3, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64), torch.tensor([40], dtype=torch.int32),
                       torch.tensor([50], dtype=torch.int32), (np.array([40]), np.array([50])))
    for t in (C.RandomResizedCrop(size=16), C.SrcCrop(size=16), C.EvalTransform(size=16)):
        with pytest.raises(TypeError, match="no CPU path"):
            t.apply(cpu)
        with pytest.raises(TypeError, match="PackedImages"):
            t.apply(torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
        with pytest.raises(TypeError, match="no CPU path"):
            t.launch(cpu.data, torch.zeros(1, 20, dtype=torch.int32), torch.zeros(8, dtype=torch.int32))
    with pytest.raises(TypeError, match="no CPU path"):
        ThreeAugment(crop=C.RandomResizedCrop(size=16)).apply_sources(cpu)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.crop_resize_u8(cpu.data, torch.zeros(1, 20, dtype=torch.int32), torch.zeros(8, dtype=torch.int32), (0, 0, 0), (1, 1, 1),
                           torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    # a resized side below the crop
    with pytest.raises(ValueError, match="below `size`"):
        C.EvalTransform(size=224, crop_ratio=1.25)
    with pytest.raises(ValueError, match="below `size`"):
        C.EvalTransform(size=224, resize_size=200)
    assert C.EvalTransform(size=224, crop_ratio=1.0).resize_size == 224
    # pad >= side
    with pytest.raises(ValueError, match="reflect padding 4"):
        C.CropParams([9], [9], 8, 8, box=[(0, 0, 9, 9)], rsize=[(4, 12)], pad=[4], win=[(0, 0)]).tables()
    with pytest.raises(ValueError, match="padding"):
        C.SrcCrop(size=16, padding=16)
    # tap counts above the kernel's
    cap = ops.crop_resize_max_taps(4096)
    assert cap < 5
    with pytest.raises(ValueError, match=f"needs 5 taps; the kernel holds {cap}"):
        C.CropParams([7], [8], 8, 4096, box=[(0, 0, 7, 8)], rsize=[(8, 4096)]).tables()
    cap = ops.crop_resize_max_taps(40)
    n = 40 * ((cap - 1) // 2 // 2) + 1                         # the first length past the cap's: 2 ceil(2 n / 40) + 1 > cap
    assert resize_taps(n - 1, 40) <= cap < resize_taps(n, 40)
    with pytest.raises(ValueError, match="taps; the kernel holds"):
        C.CropParams([n], [8], 40, 40, box=[(0, 0, n, 8)]).tables()
    C.CropParams([n - 1], [8], 40, 40, box=[(0, 0, n - 1, 8)]).tables()
    C.CropParams([8], [n], 40, 40, box=[(0, 0, 8, n)]).tables()    # the horizontal pass reads its taps from the staged source
    # boxes, windows, orientations
    for kw, msg in ((dict(box=[(0, 0, 41, 50)]), "leaves its 40 x 50 source"), (dict(box=[(0, 0, 40, 50)], win=[(1, 0)]), "window"),
                    (dict(box=[(0, 0, 40, 50)], rot=[4]), "rot must be"), (dict(box=[(0, 0, 40, 50)], rsize=[(0, 16)]), "resized to")):
        with pytest.raises(ValueError, match=msg):
            C.CropParams([40], [50], 16, 16, **kw).tables()
    with pytest.raises(ValueError, match="square output"):
        C.CropParams([40], [50], 16, 20, box=[(0, 0, 40, 50)], rot=[1]).tables()
