"""The DINOv2 multi-crop augmentation kernels (csrc/dino_augment.hip through octic_vits_amd.dino_augment) against Pillow's
recorded results (tests/golden/dino_augment.npz, made by tests/golden/make_dino_augment_golden.py from real PIL calls) and the
numpy restatement of the contract (tests/golden/dino_augment_numpy.py).  Everything but the blur is bit for bit.  The blur is
held to the rule of the contract: with e the float64 sum of the 81 products of the same f32 weights, the kernel returns rint(e)
wherever |frac(e) - 0.5| >= 2^-9 and either neighbour elsewhere (f32 accumulation of 81 non-negative terms summing to at most
255 errs by at most 81 * 2^-24 * 255 = 1.2e-3 < 2^-9), and at most 1 % of a case's pixels may be excused."""
import os
import random

import numpy as np
import pytest
import torch

import dino_augment_case as C
import dino_augment_numpy as N

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "dino_augment.npz"))
SMALL = dict(local_crops_number=2, global_crops_size=32, local_crops_size=16)


def D():
    from octic_vits_amd import dino_augment
    return dino_augment


def boxes_params(sizes, boxes, flips, S):
    """A DinoAugParams of len(boxes) sources with no local crops: global 1 is the given box and flip, global 2 its mirror."""
    box = np.stack([np.asarray(boxes, np.int32)] * 2)
    flip = np.stack([np.asarray(flips, bool), ~np.asarray(flips, bool)])
    return D().DinoAugParams([s[0] for s in sizes], [s[1] for s in sizes], 0, S, S, box=box, flip=flip)


def resize_on_device(sources, boxes, flips, S):
    aug = D().DinoAugment(global_crops_size=S, local_crops_size=S, local_crops_number=0)
    packed = D().pack_images(sources, "cuda")
    before = packed.data.clone()
    g, l = aug.apply(packed, boxes_params([s.shape[:2] for s in sources], boxes, flips, S), uint8_out=True)
    assert l.shape == (0, S, S, 3) and g.shape == (2 * len(boxes), S, S, 3) and g.dtype == torch.uint8
    assert torch.equal(packed.data, before)
    g = g.cpu().numpy()
    return g[:len(boxes)], g[len(boxes):]


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("S", [16, 12])
def test_resized_crops_equal_pils_pixels(S):
    cases = [c for c in GOLDEN["resize_cases"] if c[5] == S]
    want = GOLDEN[f"resize_out_{S}"]
    assert len(cases) == len(want) > 40
    sources = [GOLDEN[f"resize_src_{int(c[0])}"] for c in cases]
    got, mirrored = resize_on_device(sources, [c[1:5] for c in cases], [c[6] for c in cases], S)
    for i, c in enumerate(cases):
        assert np.array_equal(got[i], want[i]), c
        assert np.array_equal(mirrored[i], want[i][:, ::-1]), c
    kinds = {(int(c[3]) == S, int(c[4]) == S, int(c[3]) == 1, int(c[4]) == 1, bool(c[6])) for c in cases}
    assert len({k[:2] for k in kinds}) == 4 and any(k[2] for k in kinds) and any(k[3] for k in kinds)


def test_the_longest_tap_count_and_the_chunked_vertical_pass():
    """Sources of max_side on one axis at S = 96: 45 taps per output, and 16 output rows need more source rows than the
    kernel's LDS holds at once."""
    rs = np.random.RandomState(5)
    sources = [rs.randint(0, 256, (1024, 9, 3)).astype(np.uint8), rs.randint(0, 256, (9, 1024, 3)).astype(np.uint8)]
    boxes = [(0, 0, 1024, 9), (0, 0, 9, 1024)]
    assert D().resize_taps(1024, 96) == 45
    got, mirrored = resize_on_device(sources, boxes, [False, True], 96)
    for i in range(2):
        want = N.resized_crop(sources[i], boxes[i], 96)
        assert np.array_equal(got[i], want[:, ::-1] if i else want) and np.array_equal(mirrored[i], want if i else want[:, ::-1])


def test_ragged_batches_equal_each_source_alone():
    rs = np.random.RandomState(6)
    sources = [rs.randint(0, 256, (37, 53, 3)).astype(np.uint8), rs.randint(0, 256, (64, 48, 3)).astype(np.uint8),
               rs.randint(0, 256, (5, 5, 3)).astype(np.uint8)]
    boxes, flips = [(3, 7, 30, 41), (10, 0, 50, 48), (0, 1, 5, 3)], [True, False, True]
    both, both_m = resize_on_device(sources, boxes, flips, 16)
    for i in range(3):
        alone, alone_m = resize_on_device(sources[i:i + 1], boxes[i:i + 1], flips[i:i + 1], 16)
        assert np.array_equal(both[i], alone[0]) and np.array_equal(both_m[i], alone_m[0])
        assert np.array_equal(both[i], N.resized_crop(sources[i], boxes[i], 16)[:, ::-1] if flips[i] else N.resized_crop(sources[i], boxes[i], 16))


# ------------------------------------------------------------------------------------------------ hue
def color_rows(ps):
    """int32 [n, ROW_WORDS] for parameter dicts (the fields behind the resize)."""
    n = len(ps)
    arr = {f: np.array([[p[f] for p in ps]]) for f in ("flip", "jitter", "order", "brightness", "contrast", "saturation", "hue", "gray",
                                                      "blur", "sigma", "solarize")}
    arr = {k: np.concatenate([v, v]) for k, v in arr.items()}                         # two "crops" per source, the same
    p = D().DinoAugParams([8] * n, [8] * n, 0, 8, 8, **arr)
    return p.color_rows([(0, b) for b in range(n)])


def apply_crops(crops, ps, **kw):
    aug = D().DinoAugment()
    x = torch.from_numpy(np.ascontiguousarray(crops)).cuda()
    before = x.clone()
    out = aug.apply_crops(x, color_rows(ps), **kw)
    assert torch.equal(x, before)
    return out


@pytest.fixture(scope="module")
def all_colours():
    """All 2^24 colours as one 4096 x 4096 crop, their HSV codes and the RGB of every HSV code (numpy restatement, once)."""
    v = np.arange(1 << 24, dtype=np.uint32)
    px = np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    return px, N.rgb_to_hsv(px), N.hsv_to_rgb(px)


@pytest.mark.parametrize("factor,shift", [(0.005, 1), (0.1, 25), (-0.1, 231), (0.0, 0)])
def test_hue_on_all_colours_equals_the_restatement(all_colours, factor, shift):
    px, hsv, lut = all_colours
    assert N.hue_shift(factor) == shift
    h = (hsv[..., 0].astype(np.int64) + shift) % 256
    want = lut.reshape(256, 256, 256, 3)[h, hsv[..., 1], hsv[..., 2]]
    p = dict(C.identity((0, 0, 8, 8), 8), jitter=True, order=[3, -1, -1, -1], hue=factor)
    got = apply_crops(px[None], [p], uint8_out=True)
    assert torch.equal(got[0], torch.from_numpy(want).cuda())


def test_hue_equals_the_sampled_pil_cases():
    ps = [dict(C.identity((0, 0, 8, 8), 8), jitter=True, order=[3, -1, -1, -1], hue=float(f)) for f in GOLDEN["hue_factors"]]
    got = apply_crops(np.stack([GOLDEN["hue_src"]] * 4), ps, uint8_out=True).cpu().numpy()
    assert np.array_equal(got, GOLDEN["hue_out"])


# ------------------------------------------------------------------------------------------------ the jitter chain
@pytest.mark.parametrize("key", ["16x16", "7x30"])
def test_jitter_chain_equals_pils_pixels(key):
    ps = C.unpack(GOLDEN, f"jit_{key}_")
    assert len({tuple(p["order"]) for p in ps if p["jitter"]}) == 24
    assert {(p["gray"], p["solarize"]) for p in ps} == {(a, b) for a in (False, True) for b in (False, True)}
    src, want = GOLDEN[f"jit_src_{key}"], GOLDEN[f"jit_out_{key}"]
    got = apply_crops(src, ps, uint8_out=True).cpu().numpy()
    for i, p in enumerate(ps):
        assert np.array_equal(got[i], want[i]), (key, i, p)
    f32 = apply_crops(src, ps).cpu()
    aug = D().DinoAugment()
    assert torch.equal(f32, torch.from_numpy(N.normalize(want, aug.mean, aug.std)))


# ------------------------------------------------------------------------------------------------ blur
SIGMAS = [0.1, 0.5, 1.0, 2.0]


@pytest.mark.parametrize("shape,n", [((40, 36), 1), ((5, 5), 16)])
def test_blur_obeys_the_rounding_rule(shape, n):
    """A case is one crop shape at one sigma.  The excused share is a property of the test's own pixels (it is computed from
    the float64 sums alone, never from the kernel's output), and a share of 1 % can only be resolved on a sample of well over
    100 values: one 5 x 5 crop has 75, so that case takes 16 random 5 x 5 crops (1200 values), the 40 x 36 case one (4320).  The 1 % assertion therefore guards the test's data (that the
    band does not excuse too much of it); what is asserted of the kernel is the per-pixel rule, on every pixel."""
    rs = np.random.RandomState(8)
    H, W = shape
    crops = rs.randint(0, 256, (len(SIGMAS), n, H, W, 3)).astype(np.uint8)
    ps = [dict(C.identity((0, 0, 8, 8), 8), blur=True, sigma=s) for s in SIGMAS for _ in range(n)]
    flatc = crops.reshape(-1, H, W, 3)
    got = apply_crops(flatc, ps, uint8_out=True).cpu().numpy()
    for i, s in enumerate(SIGMAS):
        cands = [N.blur_candidates(c, N.blur_weights(s)) for c in crops[i]]
        want, alt = np.stack([c[0] for c in cands]), np.stack([c[1] for c in cands])
        have = got[i * n:(i + 1) * n]
        excused = float((want != alt).mean())
        print(f"blur {n} x {H}x{W} sigma {s}: excused {excused:.4%}, differing from rint(e) {float((have != want).mean()):.4%}")
        assert ((have == want) | (have == alt)).all(), (shape, s)
        assert excused <= 0.01, (shape, s)
    assert np.array_equal(got[:n], crops[0])                                          # sigma 0.1 returns the input
    again = apply_crops(flatc, ps, uint8_out=True).cpu().numpy()
    assert np.array_equal(got, again)                                                 # run to run
    for i in (n, 4 * n - 1):                                                          # alone and inside the batch
        alone = apply_crops(flatc[i:i + 1], ps[i:i + 1], uint8_out=True).cpu().numpy()
        assert np.array_equal(alone[0], got[i])
    flat = np.stack([np.full((H, W, 3), v, np.uint8) for v in (0, 1, 77, 255)])
    assert np.array_equal(apply_crops(flat, [ps[-1]] * 4, uint8_out=True).cpu().numpy(), flat)  # a constant crop blurs to itself
    sol = [dict(p, solarize=True) for p in ps]
    assert np.array_equal(apply_crops(flatc, sol, uint8_out=True).cpu().numpy(), N.solarize(got))


# ------------------------------------------------------------------------------------------------ the whole pipeline
def pipeline():
    dino = D()
    aug = dino.DinoAugment(generator=torch.Generator().manual_seed(5), **SMALL)
    sources = [GOLDEN[f"pipe_src_{b}"] for b in range(3)]
    packed = dino.pack_images(sources, "cuda")
    params = aug.draw(*packed.host_sizes())
    return aug, sources, packed, params


def test_pipeline_equals_the_data_augmentation_dino_oracle():
    aug, sources, packed, params = pipeline()
    before = packed.data.clone()
    assert packed.offsets.tolist() == [0, 40 * 56 * 3, 40 * 56 * 3 + 64 * 48 * 3] and packed.heights.tolist() == [40, 64, 31]
    assert packed.widths.tolist() == [56, 48, 33] and packed.data.numel() == sum(s.size for s in sources)
    g8, l8 = aug.apply(packed, params, uint8_out=True)
    g, l = aug.apply(packed, params)
    assert torch.equal(packed.data, before)
    assert g8.shape == (6, 32, 32, 3) and l8.shape == (6, 16, 16, 3) and g.shape == (6, 3, 32, 32) and l.shape == (6, 3, 16, 16)
    blurred = 0
    for b in range(3):
        ps = C.unpack(GOLDEN, f"pipe_{b}_")
        outs = list(GOLDEN[f"pipe_out_{b}_g"]) + list(GOLDEN[f"pipe_out_{b}_l"])
        for c, (p, oracle) in enumerate(zip(ps, outs)):
            assert params.crop(c, b) == dict(p, **{k: float(np.float32(p[k])) for k in ("brightness", "contrast", "saturation")})
            got = (g8[c * 3 + b] if c < 2 else l8[(c - 2) * 3 + b]).cpu().numpy()        # crop-major
            if p["blur"]:
                want, alt = N.apply_u8(sources[b], p)
                assert ((got == want) | (got == alt)).all() and (want != alt).mean() <= 0.01, (b, c)
                assert ((oracle == want) | (oracle == alt)).all()
                blurred += 1
            else:
                assert np.array_equal(got, oracle), (b, c, p)
    assert 0 < blurred < 12
    # ToTensor + Normalize of those pixels as the reference's loader runs them (torch on the host), bitwise
    mean, std = torch.tensor(aug.mean).view(3, 1, 1), torch.tensor(aug.std).view(3, 1, 1)
    for u8, f in ((g8, g), (l8, l)):
        t = u8.cpu().permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)     # ToTensor
        assert torch.equal(f.cpu(), t.sub_(mean).div_(std))                           # Normalize
    g2, l2 = aug.apply(packed, params)                                                   # run to run
    assert torch.equal(g, g2) and torch.equal(l, l2)


def test_max_side_equal_to_a_crop_size_runs_and_changes_nothing():
    """max_side fixes the capacity of the device tables only: at max_side == local_crops_size (where the pass of a full-length
    crop is skipped but every shorter crop needs five taps) the batch fits and equals the one under the default max_side."""
    dino = D()
    rs = np.random.RandomState(9)
    sources = [rs.randint(0, 256, s + (3,)).astype(np.uint8) for s in ((16, 16), (12, 16), (16, 7), (16, 16))]
    packed = dino.pack_images(sources, "cuda")
    tight = dino.DinoAugment(max_side=16, generator=torch.Generator().manual_seed(4), **SMALL)
    params = tight.draw(*packed.host_sizes())
    assert params.tables()["coef"].size <= tight.coef_capacity(4)
    wide = dino.DinoAugment(**SMALL)
    for a, b in zip(tight.apply(packed, params, uint8_out=True), wide.apply(packed, params, uint8_out=True)):
        assert torch.equal(a, b)
    for c in range(4):
        for b in range(4):
            p = params.crop(c, b)
            got = tight.apply(packed, params, uint8_out=True)[c >= 2][(c % 2) * 4 + b].cpu().numpy()
            want, alt = N.apply_u8(sources[b], p)
            assert ((got == want) | (got == alt)).all() and (p["blur"] or np.array_equal(got, want)), (c, b)


def _arch():
    from octic_vits_amd import d8_layers, dinov2_models, vit
    from octic_vits_amd import ssl as S

    def backbone():
        return dinov2_models.OcticDinoVisionTransformer(
            img_size=32, patch_size=4, embed_dim=128, depth=4, num_heads=4,
            octic_block_layers=lambda **kw: d8_layers.NestedTensorBlockD8(init_values=0.1, **{k: v for k, v in kw.items() if k != "init_values"}),
            standard_block_layers=lambda **kw: vit.NestedTensorBlock(attn_class=vit.MemEffAttention, init_values=0.1,
                                                                     **{k: v for k, v in kw.items() if k != "init_values"}))
    torch.manual_seed(0)
    arch = S.SSLMetaArch(backbone, 128, head_n_prototypes=64, head_hidden_dim=48, head_bottleneck_dim=16, local_crops_number=2)
    return S.SSLTrainer(arch.cuda().train(), lr=1e-3)


def test_collate_feeds_an_ssl_step_like_ssl_collate_on_the_same_crops():
    from octic_vits_amd import ssl as S
    aug, sources, packed, params = pipeline()
    before = packed.data.clone()
    mg = S.MaskingGenerator((8, 8), max_num_patches=32)
    random.seed(11)
    images = aug.collate(packed, (0.1, 0.5), 0.5, 64, mg, params=params)
    g, l = aug.apply(packed, params)
    random.seed(11)
    want = S.collate(g.cpu(), l.cpu(), (0.1, 0.5), 0.5, 64, mg)
    assert set(images) == set(want) and images["upperbound"] == want["upperbound"]
    for k, v in want.items():
        if torch.is_tensor(v):
            assert images[k].is_cuda and torch.equal(images[k].cpu(), v), k
    assert images["collated_global_crops"].shape == (6, 3, 32, 32) and images["collated_local_crops"].shape == (6, 3, 16, 16)
    a = _arch().step(images, teacher_temp=0.05, momentum=0.9)
    b = _arch().step({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in want.items()}, teacher_temp=0.05, momentum=0.9)
    assert set(a) == set(b) and len(a) >= 3
    for k in a:
        assert torch.isfinite(a[k]).all() and float(a[k].detach()) == float(b[k].detach()), k
    assert torch.equal(packed.data, before)
