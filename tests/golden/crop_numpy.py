"""The contract of csrc/crop.hip restated with numpy: what the kernel must compute and what Pillow / torchvision compute for the
DeiT-III crops, the evaluation resize and the quarter turns of --rot-eval (tests/golden/make_crop_golden.py holds it against live
PIL; tests/test_crop_host.py against the golden file).  No Pillow here: the GPU tests import this module on a machine without it.
The bicubic resample is the one of ``dino_augment_numpy``, imported, not copied.

One output's parameters (``case``, what ``octic_vits_amd.crop.CropParams.case`` returns): ``box`` (top, left, h, w), ``rsize``
(rh, rw), ``pad``, ``win`` (top, left), ``out`` (OH, OW), ``rot`` (quarter turns counter-clockwise), ``flip``."""
import numpy as np

from augment_numpy import normalize  # noqa: F401  (ToTensor + Normalize is shared)
from dino_augment_numpy import resample_last_axis


def resized_box(src, box, rsize):
    """img.crop(box).resize((rw, rh), BICUBIC): uint8 [H, W, 3] -> [rh, rw, 3]; horizontal pass, uint8, vertical pass."""
    top, left, h, w = (int(v) for v in box)
    rh, rw = (int(v) for v in rsize)
    c = np.ascontiguousarray(src[top:top + h, left:left + w]).transpose(0, 2, 1)    # [h, 3, w]
    c = resample_last_axis(c, rw).transpose(2, 1, 0)                                # [rw, 3, h]
    return np.ascontiguousarray(resample_last_axis(c, rh).transpose(2, 0, 1))       # [rh, rw, 3]


def apply_u8(src, case):
    """uint8 source [H, W, 3] and one output's parameters -> uint8 [OH, OW, 3]."""
    r = resized_box(np.asarray(src, dtype=np.uint8), case["box"], case["rsize"])
    p = int(case["pad"])
    if p:
        r = np.pad(r, ((p, p), (p, p), (0, 0)), mode="reflect")
    (wt, wl), (OH, OW) = case["win"], case["out"]
    assert 0 <= wt and 0 <= wl and wt + OH <= r.shape[0] and wl + OW <= r.shape[1], case
    out = np.rot90(r[wt:wt + OH, wl:wl + OW], int(case["rot"]))                     # counter-clockwise, as Image.rotate
    if case["flip"]:
        out = out[:, ::-1]
    return np.ascontiguousarray(out)


def pack(cases):
    """int32 [n, 14]: top left h w | rh rw | pad | win_top win_left | OH OW | rot flip | 0."""
    t = np.zeros((len(cases), 14), np.int32)
    for i, c in enumerate(cases):
        t[i, :13] = tuple(c["box"]) + tuple(c["rsize"]) + (c["pad"],) + tuple(c["win"]) + tuple(c["out"]) + (c["rot"], int(c["flip"]))
    return t


def unpack(t):
    return [dict(box=tuple(int(v) for v in r[0:4]), rsize=(int(r[4]), int(r[5])), pad=int(r[6]), win=(int(r[7]), int(r[8])),
                 out=(int(r[9]), int(r[10])), rot=int(r[11]), flip=bool(r[12])) for r in np.asarray(t)]
