"""Writes tests/golden/crop.npz: seeded uint8 sources, one parameter row per output and PIL's pixels for the windowed bicubic
resample of csrc/crop.hip (needs Pillow; the tests that read the file need none).  Every expected image comes out of ``pil_apply``:
``img.crop(box).resize((rw, rh), BICUBIC)``, ``numpy.pad(..., "reflect")`` (what torchvision's ``pad`` of a PIL image calls), the
window, ``img.rotate(90 rot)`` and ``ImageOps.mirror``.  The script asserts that the numpy restatement (``crop_numpy``) equals
live PIL on every case it writes, and that ``img.rotate`` of a square image is ``numpy.rot90`` (counter-clockwise).

    python tests/golden/make_crop_golden.py

Contents: ``src_i`` uint8 [H, W, 3]; ``cases`` int32 [n, 15] = (source | the 14 words of ``crop_numpy.pack``); ``out_S`` uint8
[n_S, S, S, 3], the outputs of size S in case order."""
import os

import numpy as np

import crop_numpy as N

SOURCES = [(37, 53), (64, 48), (20, 20), (9, 70), (1, 6)]
SIZES = (16, 17)
PAD = 4


def pil_apply(src, case):
    """One output through PIL itself."""
    from PIL import Image, ImageOps
    top, left, h, w = case["box"]
    rh, rw = case["rsize"]
    img = Image.fromarray(np.ascontiguousarray(src), "RGB").crop((left, top, left + w, top + h)).resize((rw, rh), Image.BICUBIC)
    p = case["pad"]
    if p:
        img = Image.fromarray(np.pad(np.asarray(img), ((p, p), (p, p), (0, 0)), mode="reflect"))
    (wt, wl), (OH, OW) = case["win"], case["out"]
    img = img.crop((wl, wt, wl + OW, wt + OH))
    if case["rot"]:
        img = img.rotate(90 * case["rot"])
    if case["flip"]:
        img = ImageOps.mirror(img)
    return np.asarray(img)


def resize_size(H, W, size):
    """torchvision's Resize(int)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(size * long / short)
    return (new_long, size) if W <= H else (size, new_long)


def case(box, rsize, S, pad=0, win=(0, 0), rot=0, flip=False):
    return dict(box=tuple(box), rsize=tuple(rsize), pad=pad, win=tuple(win), out=(S, S), rot=rot, flip=flip)


def cases_for(H, W, S, i):
    out = []
    # RandomResizedCrop: the box resized to the output, the whole of it
    boxes = [(0, 0, H, W), (H // 3, W // 4, max(H // 2, 1), max(W // 2, 1)), (H - 1, W - 1, 1, 1)]
    if H >= S:
        boxes.append((H - S, 0, S, max(W // 3, 1)))                                     # no vertical pass
    if W >= S:
        boxes.append((0, W - S, max(H // 3, 1), S))                                     # no horizontal pass
    if H >= S and W >= S:
        boxes.append((1, 2, S, S))                                                      # neither
    out += [case(b, (S, S), S, flip=(i + j) % 2 == 1) for j, b in enumerate(boxes)]
    # evaluation: Resize(int(S / 0.875)) + CenterCrop(S), and the eight orientations on the first two sources
    rh, rw = resize_size(H, W, int(S / 0.875))
    win = (int(round((rh - S) / 2.0)), int(round((rw - S) / 2.0)))
    for rot in range(4):
        for flip in (False, True):
            if i < 2 or (rot, flip) == (i % 4, i % 2 == 0):
                out.append(case((0, 0, H, W), (rh, rw), S, win=win, rot=rot, flip=flip))
    # --src: Resize(S) + RandomCrop(S, padding=4, reflect): the first, the last and one window in between
    rh, rw = resize_size(H, W, S)
    ph, pw = rh + 2 * PAD - S, rw + 2 * PAD - S
    for win in ((0, 0), (ph, pw), (ph // 2, pw // 3), (0, pw), (ph, 0)):
        out.append(case((0, 0, H, W), (rh, rw), S, pad=PAD, win=win))
    return out


def main():
    import PIL
    from PIL import Image
    rs = np.random.RandomState(20251019)
    sq = rs.randint(0, 256, (6, 6, 3)).astype(np.uint8)
    for k in range(4):                                       # Image.rotate turns counter-clockwise, exactly, on a square image
        assert np.array_equal(np.asarray(Image.fromarray(sq).rotate(90 * k)), np.rot90(sq, k)), k
    data = {"pillow_version": np.array(PIL.__version__)}
    rows, outs = [], {S: [] for S in SIZES}
    for i, (H, W) in enumerate(SOURCES):
        src = data[f"src_{i}"] = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
        for S in SIZES:
            for c in cases_for(H, W, S, i):
                got = pil_apply(src, c)
                assert np.array_equal(got, N.apply_u8(src, c)), ((H, W), c)
                rows.append(np.concatenate([[i], N.pack([c])[0]]))
                outs[S].append(got)
    data["cases"] = np.array(rows, np.int32)
    for S in SIZES:
        data[f"out_{S}"] = np.stack(outs[S])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "crop.npz")
    np.savez_compressed(path, **data)
    print(f"{path}: {len(rows)} cases, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
