"""Writes tests/golden/dino_augment.npz: inputs, parameters and PIL's results for the DINOv2 multi-crop augmentation kernels
(needs Pillow; the tests that read the file need none).  Every expected image comes out of ``dino_augment_case``, i.e. real PIL
calls plus the restated torchvision glue.  The script asserts that the numpy restatement (``dino_augment_numpy``) equals live
PIL on every case it writes, that the two colour conversions equal PIL's on all 2^24 colours in both directions, and that the
oracle's blur (torch's conv2d) obeys the rounding rule of the blur test.

    python tests/golden/make_dino_augment_golden.py

Contents: ``resize_src_i`` uint8 [H, W, 3], ``resize_cases`` int32 [n, 7] = (source, top, left, h, w, S, flip), ``resize_out_S``
uint8 [n_S, S, S, 3] in case order; ``hue_src`` uint8 [64, 64, 3], ``hue_factors`` [4], ``hue_out`` uint8 [4, 64, 64, 3];
``jit_src_K`` / ``jit_out_K`` uint8 [n, H, W, 3] and the parameters ``jit_K_<field>`` for K = 16x16, 7x30; ``pipe_src_b``, the
drawn parameters ``pipe_b_<field>`` and ``pipe_out_b_g`` [2, 32, 32, 3], ``pipe_out_b_l`` [2, 16, 16, 3] for three sources."""
import itertools
import os

import numpy as np
import torch

import dino_augment_case as C
import dino_augment_numpy as N

RESIZE_SOURCES = [(37, 53), (64, 48), (9, 200), (5, 5)]
RESIZE_SIZES = (16, 12)
HUE_FACTORS = [0.005, 0.1, -0.1, 0.0]                      # H += 1, 25, -25 (231), 0
JITTER_SHAPES = [(16, 16), (7, 30)]
PIPE_SOURCES = [(40, 56), (64, 48), (31, 33)]
PIPE_SEED = 5
PIPE_GEOMETRY = dict(local_crops_number=2, global_crops_size=32, local_crops_size=16)


def resize_boxes(H, W, S):
    """(top, left, h, w): the full image, 1-pixel crops, up- and downscaling, the skipped passes, every border."""
    boxes = [(0, 0, H, W), (0, W // 2, H, 1), (H // 2, 0, 1, W), (0, 0, 1, 1), (H - 1, W - 1, 1, 1)]
    if H >= 5 and W >= 7:
        boxes += [(H - 5, W - 7, 5, 7), (0, 0, 5, 7)]                                   # upscaling 5 x 7 -> S
    if W >= S:
        boxes += [(0, W - S, min(H, 7), S), (0, 0, H, S)]                               # w == S: no horizontal pass
    if H >= S:
        boxes += [(H - S, 0, S, min(W, 9)), (0, 0, S, W)]                               # h == S: no vertical pass
    if H >= S and W >= S:
        boxes += [(1, 2, S, S)]                                                         # both skipped
    boxes += [(0, 0, max(H // 2, 1), max(W // 2, 1)), (H - max(H // 2, 1), W - max(W // 2, 1), max(H // 2, 1), max(W // 2, 1)),
              (0, W - max(W // 3, 1), H, max(W // 3, 1)), (H - max(H // 3, 1), 0, max(H // 3, 1), W)]
    return boxes


def all_colours():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(v >> 16) & 255, (v >> 8) & 255, v & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)


def check_conversions():
    from PIL import Image
    px = all_colours()
    assert np.array_equal(np.asarray(Image.fromarray(px, "RGB").convert("HSV")), N.rgb_to_hsv(px)), "RGB -> HSV"
    assert np.array_equal(np.asarray(Image.fromarray(px, "HSV").convert("RGB")), N.hsv_to_rgb(px)), "HSV -> RGB"


def check_blur(rs):
    for (H, W), sigma in itertools.product([(40, 36), (5, 5)], [0.1, 0.5, 1.0, 2.0]):
        px = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        p = dict(C.identity((0, 0, H, W), 5), blur=True, sigma=sigma)
        got = C.color_chain_u8(px, p)
        want, alt = N.color_chain(px, p)
        assert ((got == want) | (got == alt)).all() and (want != alt).mean() <= 0.01, ((H, W), sigma)


def main():
    import PIL
    rs = np.random.RandomState(20250611)
    data = {"pillow_version": np.array(PIL.__version__)}
    check_conversions()
    check_blur(rs)

    # ---- resize
    cases, outs = [], {S: [] for S in RESIZE_SIZES}
    for i, (H, W) in enumerate(RESIZE_SOURCES):
        src = data[f"resize_src_{i}"] = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        for S in RESIZE_SIZES:
            for j, box in enumerate(resize_boxes(H, W, S)):
                for flip in ((0, 1) if j < 3 else ((i + j) % 2,)):
                    p = dict(C.identity(box, S), flip=bool(flip))
                    out = C.apply_u8(src, p)
                    want, alt = N.apply_u8(src, p)
                    assert np.array_equal(out, want) and np.array_equal(want, alt), ((H, W), p)
                    cases.append((i,) + tuple(box) + (S, flip))
                    outs[S].append(out)
    data["resize_cases"] = np.array(cases, np.int32)
    for S in RESIZE_SIZES:
        data[f"resize_out_{S}"] = np.stack(outs[S])

    # ---- hue
    hue_src = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    hue_src[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 0, 0], [254, 255, 255], [128, 128, 127]]
    data["hue_src"], data["hue_factors"] = hue_src, np.array(HUE_FACTORS)
    hue_out = []
    for f in HUE_FACTORS:
        p = dict(C.identity((0, 0, 64, 64), 64), jitter=True, order=[3, -1, -1, -1], hue=f)
        hue_out.append(C.color_chain_u8(hue_src, p))
        assert np.array_equal(hue_out[-1], N.color_chain(hue_src, p)[0]), f
    data["hue_out"] = np.stack(hue_out)
    assert [N.hue_shift(f) for f in HUE_FACTORS] == [1, 25, 231, 0]

    # ---- the jitter chain: all 24 orders, grayscale / solarize on and off, flat and two-level images
    perms = [list(p) for p in itertools.permutations(range(4))]
    for H, W in JITTER_SHAPES:
        key = f"{H}x{W}"
        srcs, ps = [], []
        fac = lambda lo, hi: float(np.float32(rs.uniform(lo, hi)))
        for i, perm in enumerate(perms):
            srcs.append(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
            ps.append(dict(C.identity((0, 0, H, W), 5), jitter=True, order=perm, brightness=fac(0.6, 1.4), contrast=fac(0.6, 1.4),
                           saturation=fac(0.8, 1.2), hue=fac(-0.1, 0.1), gray=i % 4 == 1, solarize=i % 3 == 1))
        two = (rs.randint(0, 2, (H, W, 1)) * np.array([200, 255, 13])).astype(np.uint8)
        for px in (np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), two):
            for k, perm in enumerate(([1, 3, 0, 2], [2, 0, 3, 1])):
                srcs.append(px)
                ps.append(dict(C.identity((0, 0, H, W), 5), jitter=True, order=perm, brightness=1.3, contrast=0.7 if k else 1.3,
                               saturation=1.2, hue=0.07, gray=False, solarize=bool(k)))
        srcs.append(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))                      # no jitter, grayscale and solarize
        ps.append(dict(C.identity((0, 0, H, W), 5), gray=True, solarize=True))
        outs = []
        for px, p in zip(srcs, ps):
            outs.append(C.color_chain_u8(px, p))
            assert np.array_equal(outs[-1], N.color_chain(px, p)[0]), (key, p)
        data[f"jit_src_{key}"], data[f"jit_out_{key}"] = np.stack(srcs), np.stack(outs)
        for f, v in C.pack(ps).items():
            data[f"jit_{key}_{f}"] = v

    # ---- the whole pipeline: DataAugmentationDINO on three small sources, one shared generator
    g = torch.Generator().manual_seed(PIPE_SEED)
    seen = dict(blur=0, sharp=0, jitter=0, gray=0, solarize=0, flip=0)
    for b, (H, W) in enumerate(PIPE_SOURCES):
        src = data[f"pipe_src_{b}"] = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        crops = C.draw_image(H, W, generator=g, **PIPE_GEOMETRY)
        outs = []
        for p in crops:
            out = C.apply_u8(src, p)
            want, alt = N.apply_u8(src, p)
            assert ((out == want) | (out == alt)).all() and (want != alt).mean() <= 0.01, (b, p)
            if not p["blur"]:
                assert np.array_equal(want, alt)
            outs.append(out)
            seen["blur"] += p["blur"]
            seen["sharp"] += not p["blur"]
            for f in ("jitter", "gray", "solarize", "flip"):
                seen[f] += p[f]
        data[f"pipe_out_{b}_g"], data[f"pipe_out_{b}_l"] = np.stack(outs[:2]), np.stack(outs[2:])
        for f, v in C.pack(crops).items():
            data[f"pipe_{b}_{f}"] = v
    data["pipe_generator_state"] = g.get_state().numpy()
    assert all(seen.values()), seen

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dino_augment.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(cases)} resize cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}, pipeline {seen}")


if __name__ == "__main__":
    main()
