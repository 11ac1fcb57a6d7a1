"""CPU-only: the host side of octic_vits_amd.augment - the arithmetic contract of csrc/augment.hip (restated with numpy in
tests/golden/augment_numpy.py) against PIL's recorded results (tests/golden/augment.npz) and against live PIL, draw parity with
the reference pipeline's order (tests/golden/augment_case.py), the packed table, argument validation of the C entry points and
the refusals.  Everything is bit for bit: no tolerance anywhere."""
import os
import random

import numpy as np
import pytest
import torch

import augment_case
import augment_numpy
from octic_vits_amd import _lib
from octic_vits_amd.augment import (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, AugParams, ThreeAugment, blur_constants,
                                    to_tensor)

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "augment.npz"))
KEYS = [f"{h}x{w}" for h, w in GOLDEN["shapes"]]
FIELDS = ("flip", "op", "radius", "order", "brightness", "contrast", "saturation")


def golden_params(key):
    return AugParams(*[GOLDEN[f"{f}_{key}"] for f in FIELDS])


def row_dict(p, i):
    return dict(flip=bool(p.flip[i]), op=int(p.op[i]), radius=float(p.radius[i]), order=[int(v) for v in p.order[i]],
                brightness=float(p.brightness[i]), contrast=float(p.contrast[i]), saturation=float(p.saturation[i]))


def test_golden_covers_what_it_should():
    assert KEYS == ["16x16", "7x30", "33x5", "1x9", "3x3", "40x36"]
    radii, orders, ops_flips = set(), set(), set()
    for key in KEYS:
        p = golden_params(key)
        radii |= set(p.radius[p.op == 3].tolist())
        orders |= {tuple(o) for o in p.order.tolist()}
        ops_flips |= set(zip(p.op.tolist(), p.flip.tolist()))
        assert GOLDEN["src_" + key].shape == GOLDEN["out_" + key].shape == (len(p),) + tuple(int(v) for v in key.split("x")) + (3,)
    assert radii == {0.1, 0.5, 0.9, 1.0, 1.3, 1.41, 1.42, 2.0}
    assert len([o for o in orders if sorted(o) == [-1, 0, 1, 2]]) == 24 and (-1, -1, -1, -1) in orders
    assert ops_flips == {(o, f) for o in range(4) for f in (False, True)}


@pytest.mark.parametrize("key", KEYS)
def test_numpy_restatement_equals_the_golden_bit_for_bit(key):
    p, src, want = golden_params(key), GOLDEN["src_" + key], GOLDEN["out_" + key]
    for i in range(len(p)):
        got = augment_numpy.apply_u8(src[i], row_dict(p, i))
        assert np.array_equal(got, want[i]), (key, i, row_dict(p, i))


def test_numpy_restatement_equals_live_pil():
    pytest.importorskip("PIL")
    rs = np.random.RandomState(7)
    perms = [o for key in KEYS for o in GOLDEN["order_" + key].tolist()]
    for it, (H, W) in enumerate([(16, 16), (7, 30), (33, 5), (1, 9), (3, 3), (1, 1), (2, 13), (64, 48)] * 12):
        px = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        p = dict(flip=bool(rs.randint(2)), op=it % 4, radius=float(rs.uniform(0.1, 2.0)), order=perms[rs.randint(len(perms))],
                 brightness=float(np.float32(rs.uniform(0.7, 1.3))), contrast=float(np.float32(rs.uniform(0.7, 1.3))),
                 saturation=float(np.float32(rs.uniform(0.7, 1.3))))
        assert np.array_equal(augment_numpy.apply_u8(px, p), augment_case.apply_u8(px, p)), ((H, W), p)


def test_normalize_restatement_is_torchs_to_tensor_and_normalize():
    u8 = np.arange(256, dtype=np.uint8).repeat(3).reshape(1, 16, 16, 3)
    mean, std = torch.tensor(IMAGENET_DEFAULT_MEAN), torch.tensor(IMAGENET_DEFAULT_STD)
    want = ((torch.from_numpy(u8).float() / 255 - mean) / std).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(torch.from_numpy(augment_numpy.normalize(u8, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)), want)
    aug = ThreeAugment()
    assert aug.mean == tuple(float(v) for v in mean) and aug.std == tuple(float(v) for v in std)


# ------------------------------------------------------------------------------------------------ the draw
@pytest.mark.parametrize("jitter", [0.3, 0.4, None, 0])
def test_draws_match_the_reference_order_variate_for_variate(jitter):
    B, rounds = 16, 6
    ours_rng, ref_rng = random.Random(41), random.Random(41)
    ours_gen, ref_gen = torch.Generator().manual_seed(43), torch.Generator().manual_seed(43)
    aug = ThreeAugment(color_jitter=jitter, rng=ours_rng, generator=ours_gen)
    seen_ops = set()
    for _ in range(rounds):
        got = aug.draw(B)
        for i in range(B):
            want = augment_case.draw_sample(color_jitter=jitter, rng=ref_rng, generator=ref_gen)
            have = row_dict(got, i)
            want = dict(want, **{k: float(np.float32(want[k])) for k in ("brightness", "contrast", "saturation")})
            assert have == want, (i, have, want)
            seen_ops.add(have["op"])
            if not jitter:
                assert have["order"] == [-1] * 4 and have["brightness"] == have["contrast"] == have["saturation"] == 1.0
            else:
                assert sorted(have["order"]) == [-1, 0, 1, 2]
                assert all(max(0.0, 1 - jitter) <= have[k] <= 1 + jitter for k in ("brightness", "contrast", "saturation"))
    assert seen_ops == {1, 2, 3}                         # RandomChoice always picks one of the three
    assert ours_rng.getstate() == ref_rng.getstate()
    assert torch.equal(ours_gen.get_state(), ref_gen.get_state())


def test_default_streams_are_the_modules_own():
    random.seed(5)
    torch.manual_seed(6)
    a = ThreeAugment().draw(4)
    state = random.getstate()
    random.seed(5)
    b = ThreeAugment(generator=torch.Generator().manual_seed(6)).draw(4)
    assert a == b and random.getstate() == state
    assert ThreeAugment(rng=random.Random(5), generator=torch.Generator().manual_seed(6)).draw(4) == a
    assert random.getstate() == state                    # a private stream leaves the module's alone


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("key", KEYS)
def test_table_packing_and_blur_constants(key):
    p = golden_params(key)
    t = p.table()
    assert t.dtype == np.int32 and t.shape == (len(p), 16)
    assert np.array_equal(t[:, 0], p.flip) and np.array_equal(t[:, 1], p.op)
    blur = GOLDEN["blur_" + key]
    assert np.array_equal(t[:, 2:5], blur) and (p.op == 3).any()
    for i in np.nonzero(p.op == 3)[0]:
        r, ww, fw = blur[i]
        assert blur_constants(p.radius[i]) == (r, ww, fw) and r in (0, 1) and (2 * r + 1) * ww + 2 * fw in ((1 << 24), (1 << 24) - 1)
    assert np.array_equal(t[:, 5:9], p.order)
    assert np.array_equal(t[:, 9:12].view(np.float32), np.stack([p.brightness, p.contrast, p.saturation], 1))
    assert not t[:, 12:].any()


def test_blur_constants_need_float32():
    """The stored constants are the float32 ones: the box radius computed in float64 and rounded once gives another weight at
    one of the golden radii at least (and PIL's image is then missed by up to 2)."""
    assert blur_constants(0.1)[0] == 0 and blur_constants(1.41)[0] == 0 and blur_constants(1.42)[0] == 1 and blur_constants(2.0)[0] == 1

    def f64(radius):
        s2 = radius * radius / 3
        L = np.sqrt(12 * s2 + 1)
        l = np.floor((L - 1) / 2)
        fr = np.float32(l + (2 * l + 1) * (l * (l + 1) - 3 * s2) / (6 * (s2 - (l + 1) * (l + 1))))
        return int(np.float32(np.float32(1 << 24) / np.float32(np.float32(fr * np.float32(2)) + np.float32(1))))
    assert [r for r in (0.9, 1.0, 1.3) if f64(r) != blur_constants(r)[1]]


def test_identity_and_validation_of_params():
    p = AugParams.identity(3)
    t = p.table()
    assert not t[:, :5].any() and (t[:, 5:9] == -1).all() and (t[:, 9:12].view(np.float32) == 1).all()
    p.order[0] = [3, 0, 7, 1]                             # hue and anything unknown are skipped
    assert p.table()[0, 5:9].tolist() == [-1, 0, -1, 1]
    p.op[1], p.radius[1] = 3, 2.5
    with pytest.raises(ValueError, match="radius"):
        p.table()
    p.op[1] = 4
    with pytest.raises(ValueError, match="op must be"):
        p.table()
    with pytest.raises(ValueError):
        AugParams(np.zeros(2), np.zeros(3), np.zeros(2), np.zeros((2, 4)), np.ones(2), np.ones(2), np.ones(2))


# ------------------------------------------------------------------------------------------------ ABI and refusals
def test_abi_argument_validation_without_gpu():
    """Rejected arguments return the documented negative codes before any launch; the ABI version did not move."""
    L = _lib.lib()
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    ESHAPE, EALIGN, EDTYPE, ENULL = -1, -2, -3, -4
    assert L.octic_augment_workspace_bytes(64, 224, 224) == 64 * 7 * 4 * 4
    assert L.octic_augment_workspace_bytes(1, 1, 1) == 4 and L.octic_augment_workspace_bytes(2, 33, 65) == 2 * 2 * 2 * 4
    assert L.octic_augment_workspace_bytes(0, 8, 8) == ESHAPE and L.octic_augment_workspace_bytes(1, -8, 8) == ESHAPE
    src, dst, tab, ws = 1 << 20, 2 << 20, 3 << 20, 4 << 20
    call = lambda **k: L.octic_augment_u8(*[k.get(n, v) for n, v in (
        ("src", src), ("dst", dst), ("dtype", _lib.F32), ("table", tab), ("m0", 0.5), ("m1", 0.5), ("m2", 0.5), ("s0", 0.25),
        ("s1", 0.25), ("s2", 0.25), ("B", 2), ("H", 8), ("W", 8), ("ws", ws), ("stream", None))])
    assert call(src=None) == ENULL and call(dst=None) == ENULL and call(table=None) == ENULL and call(ws=None) == ENULL
    assert call(B=0) == ESHAPE and call(H=0) == ESHAPE and call(W=-3) == ESHAPE
    assert call(H=1 << 15, W=1 << 15) == ESHAPE                                              # H W 3 >= 2^31
    assert call(H=26755, W=26755) == ESHAPE and call(H=1 << 30, W=1) == ESHAPE
    assert call(dtype=_lib.BF16) == EDTYPE and call(dtype=9) == EDTYPE
    assert call(dst=dst + 2) == EALIGN and call(table=tab + 2) == EALIGN and call(ws=ws + 1) == EALIGN
    nin = 2 * 8 * 8 * 3
    for d in (src, src + 4, src + nin - 4, src - 4 * nin + 4):                               # overlapping src / f32 dst
        assert call(dst=d) == ESHAPE
    for d in (src, src + 1, src + nin - 1, src - nin + 1):                                   # overlapping src / uint8 dst
        assert call(dst=d, dtype=_lib.U8) == ESHAPE


def test_cpu_tensors_and_wrong_batches_are_refused():
    aug = ThreeAugment()
    x = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    for fn in (aug.apply, aug.to_tensor, aug, to_tensor):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(x)
    for bad in (torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8, dtype=torch.uint8), torch.zeros(8, 8, 3, dtype=torch.uint8), None):
        with pytest.raises(TypeError, match=r"uint8 \[B, H, W, 3\]"):
            aug.apply(bad)
    from octic_vits_amd.train import evaluate
    with pytest.raises(RuntimeError, match="GPU only"):
        evaluate(torch.nn.Linear(3, 3), [(x, torch.zeros(2, dtype=torch.int64))])
    with pytest.raises(ValueError):
        ThreeAugment(color_jitter=-0.1)
    with pytest.raises(ValueError):
        ThreeAugment(mean=(0.5, 0.5))


def test_trainer_with_augment_refuses_the_cpu_and_segment_graphs():
    from octic_vits_amd.model import OcticVisionTransformer
    from octic_vits_amd.train import Trainer
    net = OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=2, num_heads=2,
                                 mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=1)
    with pytest.raises(RuntimeError, match=r"augment=.*GPU only"):
        Trainer(net, augment=ThreeAugment(), fused_optimizer=False)
    with pytest.raises(RuntimeError, match="segment_graphs"):
        Trainer(net, augment=ThreeAugment(), fused_optimizer=False, device_type="cuda", segment_graphs=2)
    tr = Trainer(net, fused_optimizer=False)              # augment=None: nothing about the trainer changes
    assert tr.augment is None and tr.mixup is None
