"""The windowed bicubic resample of csrc/crop.hip (through octic_vits_amd.crop, ThreeAugment(crop=...), Trainer and
train.evaluate) on the GPU, against the numpy restatement of the contract (tests/golden/crop_numpy.py, which the golden maker and
tests/test_crop_host.py hold against PIL) and PIL's recorded pixels (tests/golden/crop.npz).  Every comparison is bitwise.  Output
sizes run from 5 to 40 and sit on both sides of the kernel's tile of window rows, which is read from the library."""
import os
import random

import numpy as np
import pytest
import torch

import crop_numpy as N
from octic_vits_amd import augment as A
from octic_vits_amd import crop as C
from octic_vits_amd import dino_augment as D
from octic_vits_amd import ops
from octic_vits_amd.mixup import Mixup

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "crop.npz"))
R = ops.crop_resize_rows()
SIZES = sorted({5, R - 1, R, R + 1, 2 * R + 1, 40})
MEAN = tuple(float(np.float32(v)) for v in A.IMAGENET_DEFAULT_MEAN)
STD = tuple(float(np.float32(v)) for v in A.IMAGENET_DEFAULT_STD)


def image(rs, H, W):
    return rs.randint(0, 256, (H, W, 3)).astype(np.uint8)


def launch(sources, params, f32=False, guard=0):
    """The kernel on host tables: uint8 [N, OH, OW, 3] or f32 [N, 3, OH, OW] as numpy (and the guard bands round the output)."""
    packed = D.pack_images(sources, "cuda")
    before = packed.data.clone()
    t = params.tables()
    rows, coef = torch.from_numpy(t["rows"]).cuda(), torch.from_numpy(t["coef"]).cuda()
    n, OH, OW = len(params), params.out_h, params.out_w
    shape, dt, fill = ((n, 3, OH, OW), torch.float32, 7.5) if f32 else ((n, OH, OW, 3), torch.uint8, 0xA5)
    numel = n * OH * OW * 3
    buf = torch.full((numel + 2 * guard,), fill, dtype=dt, device="cuda")
    out = ops.crop_resize_u8(packed.data, rows, coef, MEAN, STD, buf[guard:guard + numel].view(shape))
    assert torch.equal(packed.data, before)
    if guard:
        return out.cpu().numpy(), buf[:guard].cpu().numpy(), buf[guard + numel:].cpu().numpy()
    return out.cpu().numpy()


def want_of(sources, params):
    return np.stack([N.apply_u8(sources[int(params.source[i])], params.case(i)) for i in range(len(params))])


def check(sources, params):
    want = want_of(sources, params)
    got = launch(sources, params)
    for i in range(len(params)):
        assert np.array_equal(got[i], want[i]), params.case(i)
    got = launch(sources, params, f32=True)
    assert got.dtype == np.float32 and np.array_equal(got, N.normalize(want, MEAN, STD))
    return want


def params_of(sources, S, entries, OW=None):
    """entries: (source, box, rsize or None, pad, win, rot, flip) per output."""
    return C.CropParams([s.shape[0] for s in sources], [s.shape[1] for s in sources], S, OW or S, box=[e[1] for e in entries],
                        source=[e[0] for e in entries], rsize=[e[2] or (S, OW or S) for e in entries], pad=[e[3] for e in entries],
                        win=[e[4] for e in entries], rot=[e[5] for e in entries], flip=[e[6] for e in entries])


# ------------------------------------------------------------------------------------------------ the three modes
@pytest.mark.parametrize("S", SIZES)
def test_rrc_mode_equals_the_restatement_and_the_parents_kernel(S):
    """The full window of a box resized to S x S: a side of 1, sides below S (5 taps), the skipped pass on either axis alone and
    on both, down- and upscaling boxes, mirrored and not - and the same boxes through octic_dino_resize_u8."""
    rs = np.random.RandomState(S)
    sources = [image(rs, 1, 9), image(rs, 9, 1), image(rs, 3, 4), image(rs, S, 23), image(rs, 23, S), image(rs, S, S), image(rs, 37, 53)]
    boxes = [(0, (0, 0, 1, 9)), (1, (0, 0, 9, 1)), (0, (0, 4, 1, 1)), (2, (0, 0, 3, 4)), (3, (0, 0, S, 23)), (3, (0, 3, S, 2)),
             (4, (0, 0, 23, S)), (4, (20, 0, 3, S)), (5, (0, 0, S, S)), (6, (0, 0, 37, 53)), (6, (5, 7, 30, 41)), (6, (30, 50, 7, 3))]
    entries = [(s, b, None, 0, (0, 0), 0, bool((i + S) % 2)) for i, (s, b) in enumerate(boxes)]
    p = params_of(sources, S, entries)
    want = check(sources, p)
    # the parent's kernel: one source per crop there, so the sources are repeated
    per = [sources[s] for s, _ in boxes]
    box = np.stack([np.asarray([b for _, b in boxes], np.int32)] * 2)
    flip = np.stack([p.flip, p.flip])
    dp = D.DinoAugParams([s.shape[0] for s in per], [s.shape[1] for s in per], 0, S, S, box=box, flip=flip)
    g, _ = D.DinoAugment(global_crops_size=S, local_crops_size=S, local_crops_number=0).apply(D.pack_images(per, "cuda"), dp, uint8_out=True)
    assert np.array_equal(g[:len(boxes)].cpu().numpy(), want)


@pytest.mark.parametrize("S", SIZES)
def test_eval_mode_equals_the_restatement(S):
    """Resize + CenterCrop: a window strictly inside a non-square resized image, portrait and landscape, odd and even margins."""
    rs = np.random.RandomState(100 + S)
    sources = [image(rs, 45, 31), image(rs, 31, 45), image(rs, 2 * S + 3, S + 2), image(rs, S, 3 * S), image(rs, 7, 7)]
    hs, ws = [s.shape[0] for s in sources], [s.shape[1] for s in sources]
    for kw in (dict(crop_ratio=0.875), dict(resize_size=S + 3), dict(resize_size=S + 4)):
        p = C.EvalTransform(size=S, **kw).draw(hs, ws)
        assert (p.rsize[:, 0] != p.rsize[:, 1]).any()
        if "resize_size" in kw:
            assert (p.win.max(1) >= 2).all() and {int(v) for v in p.rsize.min(1)} == {kw["resize_size"]}
        check(sources, p)


@pytest.mark.parametrize("S", SIZES)
def test_src_mode_equals_the_restatement(S):
    """Resize(S) + RandomCrop(S, padding=4, reflect): windows at offset 0 and at the largest offset on both axes - every output
    corner reads reflected pixels - and a resized side of exactly S."""
    rs = np.random.RandomState(200 + S)
    sources = [image(rs, S, S), image(rs, S, 2 * S + 3), image(rs, 30, 21), image(rs, 3, 5)]
    entries = []
    for s, src in enumerate(sources):
        rh, rw = C.resize_size(src.shape[0], src.shape[1], S)
        assert min(rh, rw) == S
        my, mx = rh + 8 - S, rw + 8 - S
        for win in ((0, 0), (my, mx), (0, mx), (my, 0), (my // 2, mx // 2)):
            entries.append((s, (0, 0) + src.shape[:2], (rh, rw), 4, win, 0, False))
    assert sources[0].shape[:2] == (S, S)                         # no pass at all: the window reads the source and its reflection
    check(sources, params_of(sources, S, entries))
    # ... and SrcCrop's own draw
    p = C.SrcCrop(size=S, generator=torch.Generator().manual_seed(S)).draw([s.shape[0] for s in sources], [s.shape[1] for s in sources])
    assert (p.pad == 4).all()
    check(sources, p)


@pytest.mark.parametrize("S", [R - 1, R + 1])
def test_all_eight_orientations(S):
    rs = np.random.RandomState(300 + S)
    sources = [image(rs, 29, 41)]
    rh, rw = C.resize_size(29, 41, S + 2)
    entries = []
    for rot in range(4):
        for flip in (False, True):
            entries.append((0, (0, 0, 29, 41), (rh, rw), 0, (1, C.center_crop_offset(rw, S)), rot, flip))     # evaluation
            entries.append((0, (3, 5, 20, 30), None, 0, (0, 0), rot, flip))                                     # a resized box
            entries.append((0, (0, 0, 29, 41), C.resize_size(29, 41, S), 4, (8, 3), rot, flip))                 # reflected corners
    p = params_of(sources, S, entries)
    want = check(sources, p)
    assert len({want[i].tobytes() for i in range(0, len(entries), 3)}) == 8     # the image is asymmetric: eight different results
    # the transform's own draws: RandomRotate90 from Python's random, then the mirror
    ev = C.EvalTransform(size=S, rot=True, flip=True, rng=random.Random(S))
    q = ev.draw([29] * 8, [41] * 8)
    assert len(set(q.rot.tolist())) > 1
    check([sources[0]] * 8, q)


def test_non_square_outputs():
    """OH != OW (rot 0 and 2): rows whose byte count is no multiple of four, more than one tile of rows."""
    rs = np.random.RandomState(7)
    sources = [image(rs, 50, 33)]
    for OH, OW in ((7, 18), (2 * R + 3, 5), (5, 39)):
        entries = [(0, (0, 0, 50, 33), (OH + 6, OW + 9), 0, (3, 4), rot, flip) for rot in (0, 2) for flip in (False, True)]
        entries += [(0, (2, 1, 40, 30), (OH, OW), 4, (0, 8), 0, True), (0, (2, 1, 40, 30), (OH, OW), 3, (6, 0), 2, False)]
        check(sources, params_of(sources, OH, entries, OW=OW))


def test_the_largest_tap_counts_and_wide_sources():
    """At OW = 40 the kernel's LDS holds 409 rows: a source of 4080 rows needs exactly that many taps per output row (one window
    row per chunk), one of 4060 the count below (407); on the other axis the same lengths as row segments in LDS, and a source
    wider than the staging buffer, which is read from memory directly."""
    S, cap = 40, ops.crop_resize_max_taps(40)
    assert D.resize_taps(4080, S) == cap == 409 and D.resize_taps(4060, S) == cap - 2
    rs = np.random.RandomState(9)
    sources = [image(rs, 4080, 3), image(rs, 4060, 2), image(rs, 3, 4080), image(rs, 2, 4060), image(rs, 2, 4200), image(rs, 900, 4)]
    entries = [(s, (0, 0) + src.shape[:2], None, 0, (0, 0), 0, bool(s % 2)) for s, src in enumerate(sources)]
    entries.append((4, (0, 0, 2, 4200), (S, S + 30), 4, (3, 38), 0, False))       # the window's columns only, wide source
    entries.append((5, (0, 0, 900, 4), (S + 30, S), 0, (17, 0), 2, False))        # chunks of several rows
    check(sources, params_of(sources, S, entries))
    with pytest.raises(ValueError, match="taps; the kernel holds 409"):
        params_of([image(rs, 4081, 1)], S, [(0, (0, 0, 4081, 1), None, 0, (0, 0), 0, False)]).tables()


# ------------------------------------------------------------------------------------------------ PIL's recorded pixels
@pytest.mark.parametrize("S", [16, 17])
def test_the_kernel_equals_pils_recorded_pixels(S):
    rows = [r for r in GOLDEN["cases"] if r[10] == S]
    cases = N.unpack(np.asarray(rows)[:, 1:])
    want = GOLDEN[f"out_{S}"]
    assert len(cases) == len(want) > 50
    sources = [GOLDEN[f"src_{i}"] for i in range(5)]
    p = params_of(sources, S, [(int(r[0]), c["box"], c["rsize"], c["pad"], c["win"], c["rot"], c["flip"]) for r, c in zip(rows, cases)])
    got = launch(sources, p)
    for i, c in enumerate(cases):
        assert np.array_equal(got[i], want[i]), c
    assert np.array_equal(launch(sources, p, f32=True), N.normalize(want, MEAN, STD))


# ------------------------------------------------------------------------------------------------ the batch
def mixed_batch(S):
    rs = np.random.RandomState(400 + S)
    sources = [image(rs, 37, 53), image(rs, 64, 48), image(rs, 5, 5), image(rs, S, S)]
    entries = [(0, (3, 7, 30, 41), None, 0, (0, 0), 0, True), (1, (0, 0, 64, 48), C.resize_size(64, 48, S + 3), 0, (2, 1), 3, False),
               (2, (0, 1, 5, 3), None, 0, (0, 0), 2, True), (3, (0, 0, S, S), (S, S), 4, (8, 0), 1, True),
               (1, (10, 0, 50, 48), C.resize_size(50, 48, S), 4, (1, 5), 0, False)]
    return sources, entries


def test_an_image_does_not_depend_on_its_place_in_the_batch_and_launches_repeat():
    S = R + 1
    sources, entries = mixed_batch(S)
    alone = [launch(sources, params_of(sources, S, [e]))[0] for e in entries]
    alone_f = [launch(sources, params_of(sources, S, [e]), f32=True)[0] for e in entries]
    for shift in range(len(entries)):
        order = entries[shift:] + entries[:shift]
        p = params_of(sources, S, order)
        got, got_f = launch(sources, p), launch(sources, p, f32=True)
        for i in range(len(order)):
            j = (i + shift) % len(entries)
            assert np.array_equal(got[i], alone[j]) and np.array_equal(got_f[i], alone_f[j]), (shift, i)
        assert np.array_equal(launch(sources, p), got) and np.array_equal(launch(sources, p, f32=True), got_f)    # a second launch


def corrupt(rows, coef_len, kind, S):
    r = rows[1]
    H, W, top, left, h, w, rh, rw, pad = (int(v) for v in r[2:11])
    if kind == "box":
        r[4] = H - h + 1                                      # top + h > src_h
    elif kind == "box_left":
        r[5] = -1
    elif kind == "source":
        r[0:2] = np.array([1 << 40], np.int64).view(np.int32)       # the source lies outside data
    elif kind == "source_size":
        r[2] = H + 100000                                     # ... or ends outside it
        r[6] = h
    elif kind == "blocks_h":
        r[15] = coef_len - 1
    elif kind == "blocks_v":
        r[18] = coef_len
    elif kind == "window":
        r[11] = rh + 2 * pad - S + 1
    elif kind == "window_left":
        r[12] = -1
    elif kind == "rot":
        r[13] = 4
    elif kind == "rot_negative":
        r[13] = -1
    elif kind == "pad":
        r[10] = min(rh, rw)
    elif kind == "pad_negative":
        r[10] = -1
    else:
        raise AssertionError(kind)


KINDS = ["box", "box_left", "source", "source_size", "blocks_h", "blocks_v", "window", "window_left", "rot", "rot_negative", "pad",
         "pad_negative"]


@pytest.mark.parametrize("f32", [False, True])
def test_a_malformed_row_gives_zeros_and_nothing_else_changes(f32):
    S = R + 1
    sources, entries = mixed_batch(S)
    entries = [entries[0], entries[4], entries[1]]             # the middle one: a window into the reflect padding
    p = params_of(sources, S, entries)
    good, lo, hi = launch(sources, p, f32=f32, guard=1024)
    sentinel = lo.copy()
    assert np.array_equal(lo, hi) and good[1].any()
    tables = p.tables()
    for kind in KINDS:
        t = {k: v.copy() for k, v in tables.items()}
        corrupt(t["rows"], t["coef"].size, kind, S)

        class Bad:                                              # the same parameters with one row spoiled behind the host's checks
            out_h, out_w = S, S
            __len__ = lambda self: 3
            tables = lambda self: t
        got, lo, hi = launch(sources, Bad(), f32=f32, guard=1024)
        assert not got[1].any(), kind
        assert np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2]), kind
        assert np.array_equal(lo, sentinel) and np.array_equal(hi, sentinel), kind


def test_odd_turns_need_a_square_output():
    rs = np.random.RandomState(11)
    sources = [image(rs, 20, 30)]
    p = params_of(sources, 8, [(0, (0, 0, 20, 30), None, 0, (0, 0), 0, False)], OW=12)
    t = p.tables()
    t["rows"][0, 13] = 1

    class Bad:
        out_h, out_w = 8, 12
        __len__ = lambda self: 1
        tables = lambda self: t
    assert not launch(sources, Bad()).any() and launch(sources, p).any()


# ------------------------------------------------------------------------------------------------ the transforms
def _sources(seed, n=8):
    rs = np.random.RandomState(seed)
    return [image(rs, int(rs.randint(20, 70)), int(rs.randint(20, 70))) for _ in range(n)]


def test_eval_transform_f32_equals_to_tensor_of_its_uint8_output():
    sources = _sources(1)
    packed = D.pack_images(sources, "cuda")
    for ev in (C.EvalTransform(size=32), C.EvalTransform(size=32, rot=True, flip=True, rng=random.Random(2)),
               C.make_classification_eval_transform(resize_size=40, crop_size=32)):
        p = ev.draw(*packed.host_sizes())
        u8 = ev.apply(packed, p, uint8_out=True)
        f = ev.apply(packed, p)
        assert u8.shape == (8, 32, 32, 3) and u8.dtype == torch.uint8 and f.shape == (8, 3, 32, 32) and f.dtype == torch.float32
        assert torch.equal(f, A.to_tensor(u8))
        assert np.array_equal(u8.cpu().numpy(), want_of(sources, p))
    twin = C.EvalTransform(size=32, rot=True, rng=random.Random(5))
    assert torch.equal(C.EvalTransform(size=32, rot=True, rng=random.Random(5))(packed), twin.apply(packed, twin.draw(*packed.host_sizes())))
    with pytest.raises(ValueError, match="other sizes"):
        ev.apply(packed, ev.draw([30] * 8, [30] * 8))
    with pytest.raises(ValueError, match="another output size"):
        ev.apply(packed, C.EvalTransform(size=16).draw(*packed.host_sizes()))


def _three(seed, crop_seed=None, src=False):
    crop = None
    if crop_seed is not None:
        crop = (C.SrcCrop(size=32, generator=torch.Generator().manual_seed(crop_seed)) if src else
                C.RandomResizedCrop(size=32, rng=random.Random(crop_seed)))
    return A.ThreeAugment(rng=random.Random(seed), generator=torch.Generator().manual_seed(seed + 1), crop=crop)


@pytest.mark.parametrize("src", [False, True])
def test_apply_sources_equals_apply_on_the_crops(src):
    sources = _sources(3)
    packed = D.pack_images(sources, "cuda")
    aug = _three(4, 5, src)
    cp, ap = aug.draw_sources(*packed.host_sizes())
    crops = aug.crop.apply(packed, cp, uint8_out=True)
    assert np.array_equal(crops.cpu().numpy(), want_of(sources, cp))
    assert torch.equal(aug.apply_sources(packed, (cp, ap)), _three(0).apply(crops, ap))
    assert torch.equal(aug.apply_sources(packed, (cp, ap), uint8_out=True), _three(0).apply(crops, ap, uint8_out=True))
    # a fresh draw: the same seeds, the same batch
    assert torch.equal(_three(4, 5, src).apply_sources(packed), aug.apply_sources(packed, (cp, ap)))


# ------------------------------------------------------------------------------------------------ the trainer
KW = dict(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=4, num_heads=2,
          mlp_ratio=4.0, drop_path_rate=0.0, octic_equi_break_layer=2)
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=10)


def _model():
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(0)
    return OcticVisionTransformer(**KW).cuda()


def _batches(n, B=8, seed=100):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(D.pack_images(_sources(seed + i, B), "cuda"), torch.randint(0, 10, (B,), generator=g, device="cuda")) for i in range(n)]


def _same_weights(ta, tb):
    for (n, pa), pb in zip(ta.raw_model.named_parameters(), tb.raw_model.parameters()):
        assert torch.equal(pa, pb), n
    for ea, eb in zip(ta.optimizer.ema_state(), tb.optimizer.ema_state()):
        assert torch.equal(ea, eb)


def test_trainer_eager_step_on_sources_equals_the_step_on_their_crops():
    """The crop has a stream of its own here, so a twin that is fed the crops (and skips the crop draws) stays in step."""
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(7), **MIX), augment=_three(3, 9))
    tb = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(7), **MIX), augment=_three(3, 10))
    crop = C.RandomResizedCrop(size=32, rng=random.Random(9))
    la, lb = [], []
    for packed, y in _batches(2):
        la.append(float(ta.step(packed, y)))
        crops = crop.apply(packed, uint8_out=True)
        lb.append(float(tb.step(crops, y)))                   # a uint8 batch is still taken, and skips the crop
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)
    with pytest.raises(TypeError, match="needs Trainer"):
        Trainer(_model(), lr=1e-3, augment=_three(1)).step(packed, y)
    with pytest.raises(TypeError, match="needs Trainer"):
        Trainer(_model(), lr=1e-3).step(packed, y)


def test_trainer_captured_step_on_sources_equals_eager():
    from octic_vits_amd.train import Trainer
    ta = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(11), **MIX), augment=_three(21, 22))
    tb = Trainer(_model(), lr=1e-3, mixup=Mixup(rng=np.random.RandomState(11), **MIX), augment=_three(21, 22))
    batches = _batches(4, seed=200)
    gs = tb.capture(*batches[0], warmup=2)
    assert gs.samples.dtype == torch.uint8 and gs.samples.shape == (8, 32, 32, 3)    # the graph's input: the uint8 staging batch
    for _ in range(2):
        ta.step(*batches[0])
    lb = [gs.replay(x, y).clone() for x, y in batches[1:]]
    la = [ta.step(x, y) for x, y in batches[1:]]
    la, lb = [float(v) for v in la], [float(v) for v in lb]
    assert la == lb, (la, lb)
    assert len(set(la)) == len(la)
    _same_weights(ta, tb)


def test_evaluate_takes_packed_sources_through_an_eval_transform():
    from octic_vits_amd.train import evaluate
    net = _model()
    batches = _batches(2, seed=300)
    ev = C.EvalTransform(size=32)
    a = evaluate(net, batches, graphed=False, transform=ev)
    b = evaluate(net, [(ev.apply(x, uint8_out=True), y) for x, y in batches], graphed=False)
    assert a == b and a["loss"] == a["loss"]
    turned = evaluate(net, batches, graphed=False, transform=C.EvalTransform(size=32, rot=True, flip=True, rng=random.Random(1)))
    assert turned["loss"] == turned["loss"]
