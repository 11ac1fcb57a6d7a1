"""What the DPT golden (tests/golden/dpt_head.npz, made by make_dpt_golden.py from the real reference) and its tests share: the
tiny backbone of depth_cases, two inputs (grids 3 x 4 and 5 x 3 - both axes of the 5 x 3 one and one of the other meet the
unequal-size skip resize), the head's fill and the calls.  Parameters are name-keyed (cases.fill_parameters), so nothing but the
reference's outputs and the list of state-dict keys is stored."""
import torch

import cases
import depth_cases as DC

SPEC, SALT, OUT_INDEX = DC.SPEC, DC.SALT, DC.OUT_INDEX[4]
HEAD_SALT = "dpt.head."
MIN_DEPTH, MAX_DEPTH = 0.001, 10.0
H2, W2 = 60, 40                   # padded to 70 x 42: a 5 x 3 grid
STRIDE, CROP = DC.STRIDE, DC.CROP


def image():
    return DC.image()


def image2():
    return cases.randn("dpt.img2", 2, 3, H2, W2)


def fill_head(head):
    """Name-keyed values, then + 1.25 on the last bias: without a shift nearly every output pixel of the reference sits on the
    min_depth clamp and a comparison sees nothing; with + 1.0 the pre-activation still dips to -0.056 at 8 border pixels of the
    raw maps - the pixels a padding mistake would move."""
    cases.fill_parameters(head, salt=HEAD_SALT)
    with torch.no_grad():
        head.conv_depth.head[4].bias.add_(1.25)
    return head


def run(model):
    """The recorded calls on a depther (the reference's or this package's), as name -> float32 array."""
    x, y = image(), image2()
    meta = DC.meta
    out = {}
    with torch.no_grad():
        out["whole"] = model.whole_inference(x, None, True)
        out["whole_raw"] = model.whole_inference(x, None, False)
        out["whole2"] = model.whole_inference(y, None, True)
        out["whole2_raw"] = model.whole_inference(y, None, False)
        out["sized"] = model.whole_inference(x, [meta()] * 2, True, size=(17, 23))
        pair = model.aug_test([x, x.flip(3)], [[meta()] * 2, [meta(True)] * 2])
        out["aug"] = torch.stack([torch.as_tensor(a) for a in pair])
        out["slide"] = model.slide_inference(x, None, True, STRIDE, CROP)
        out["simple"] = torch.stack([torch.as_tensor(a) for a in model.simple_test(x, [meta()] * 2)])
    return {k: v.float().cpu().numpy() for k, v in out.items()}
