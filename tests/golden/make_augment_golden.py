"""Writes tests/golden/augment.npz: inputs, parameter rows and PIL's results for the 3-Augment kernels (needs Pillow; the tests
that read the file need none).  Every expected image comes out of ``augment_case.apply_u8``, i.e. real PIL calls; the box
constants (r, ww, fw) stored next to the blur radii are the ones of the float32 recipe of include/octic_hip.h, kept only where
an integer restatement of the blur with them (``augment_numpy.blur``) reproduces PIL's image bit for bit - which this script
asserts for every blur case.

    python tests/golden/make_augment_golden.py

Per shape ``HxW`` the file holds ``src_HxW`` uint8 [n, H, W, 3], ``out_HxW`` uint8 [n, H, W, 3] and the parameters ``flip_``,
``op_``, ``radius_``, ``order_`` [n, 4], ``brightness_``, ``contrast_``, ``saturation_``, ``blur_`` [n, 3] = (r, ww, fw)."""
import itertools
import os

import numpy as np

import augment_case
import augment_numpy

SHAPES = [(16, 16), (7, 30), (33, 5), (1, 9), (3, 3), (40, 36)]
RADII = [0.1, 0.5, 0.9, 1.0, 1.3, 1.41, 1.42, 2.0]
PERMS = [[v if v < 3 else -1 for v in p] for p in itertools.permutations(range(4))]     # 3 = hue: None in the recipe
FIXED = [0.7, 1.0, 1.3]
OFF = [-1, -1, -1, -1]


def cases_for(shape, rs, small):
    H, W = shape
    rnd = lambda: rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    fac = lambda: float(np.float32(rs.uniform(0.7, 1.3)))
    out = []

    def add(px, flip, op, radius=0.0, order=OFF, b=1.0, c=1.0, s=1.0):
        out.append((px, dict(flip=bool(flip), op=op, radius=radius if op == 3 else 0.0, order=list(order), brightness=b,
                             contrast=c, saturation=s)))

    k = 0
    # each op with and without flip, jitter off and on
    for op in range(4):
        for flip in (0, 1):
            add(rnd(), flip, op, RADII[k % 8])
            add(rnd(), flip, op, RADII[(k + 3) % 8], PERMS[(5 * k) % 24], fac(), fac(), fac())
            k += 1
    # every blur radius, both sides of the l = 0 -> 1 switch, with and without flip
    for i, radius in enumerate(RADII if not small else RADII[2:6]):
        for flip in (0, 1):
            add(rnd(), flip, 3, radius, PERMS[(7 * i + flip) % 24] if i % 2 else OFF, fac(), fac(), fac())
    # all 24 orders of the jitter, fixed and random factors
    for i, perm in enumerate(PERMS if not small else PERMS[::6]):
        f = [FIXED[(i + j) % 3] for j in range(3)] if i % 2 == 0 else [fac(), fac(), fac()]
        add(rnd(), i % 2, i % 4, RADII[i % 8], perm, *f)
    for f in FIXED:
        add(rnd(), 0, 0, 0.0, [0, 1, 2, -1], f, f, f)
    # flat and two-level images
    two = (rs.randint(0, 2, (H, W, 1)) * np.array([200, 255, 13])).astype(np.uint8)
    for px in (np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8), two):
        add(px, 1, 3, 1.3, [1, 2, 0, -1], 1.3, 0.7, 1.3)
        if not small:
            add(px, 0, 2, 0.0, [2, -1, 1, 0], 0.7, 1.3, 0.7)
            add(px, 0, 1, 0.0, [-1, 1, 0, 2], fac(), fac(), fac())
    return out


def main():
    import PIL
    rs = np.random.RandomState(20240917)
    data = {"pillow_version": np.array(PIL.__version__), "shapes": np.array(SHAPES)}
    total = 0
    for shape in SHAPES:
        cs = cases_for(shape, rs, small=shape == (40, 36))
        key = f"{shape[0]}x{shape[1]}"
        outs, blur = [], np.zeros((len(cs), 3), np.int64)
        for i, (px, p) in enumerate(cs):
            outs.append(augment_case.apply_u8(px, p))
            if p["op"] == 3:
                blur[i] = augment_numpy.blur_constants(p["radius"])
                q = dict(p, flip=False, order=OFF)
                assert np.array_equal(augment_case.apply_u8(px, q), augment_numpy.blur(px, *blur[i])), (shape, p)
        data["src_" + key] = np.stack([c[0] for c in cs])
        data["out_" + key] = np.stack(outs)
        data["blur_" + key] = blur
        data["flip_" + key] = np.array([c[1]["flip"] for c in cs], bool)
        data["op_" + key] = np.array([c[1]["op"] for c in cs], np.int32)
        data["radius_" + key] = np.array([c[1]["radius"] for c in cs], np.float64)
        data["order_" + key] = np.array([c[1]["order"] for c in cs], np.int32)
        for name in ("brightness", "contrast", "saturation"):
            data[f"{name}_{key}"] = np.array([c[1][name] for c in cs], np.float32)
        total += len(cs)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augment.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {total} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
