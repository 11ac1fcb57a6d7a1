"""What the depth golden (tests/golden/depth_linear.npz, made by make_depth_golden.py from the real reference) and its tests share:
the tiny backbone, the input, the metas and the calls.  Parameters are name-keyed (cases.fill_parameters), so the backbone is
rebuilt from its salt and only the head's weights are stored (float16-exact values, to halve the file)."""
import torch

import cases

SPEC = dict(img_size=56, patch_size=14, embed_dim=64, depth=4, num_heads=2, init_values=1.0)
SALT = "depth.backbone."
OUT_INDEX = {4: [0, 1, 2, 3], 1: [3]}
H, W = 30, 45                     # padded to 42 x 56: a 3 x 4 grid, the odd pixel on the right / bottom
STRIDE, CROP = (14, 20), (28, 30)


def image():
    return cases.randn("depth.img", 2, 3, H, W)


def meta(flip=False):
    return dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), flip=flip, flip_direction="horizontal")


def head_weights(layers):
    """conv_depth.weight / bias of the layers-layer head: float16-exact, O(1) logits on the O(1) features."""
    C = 2 * SPEC["embed_dim"] * layers
    w = (cases.randn(f"depth.head{layers}.weight", 256, C, 1, 1) * (2.0 / C ** 0.5)).half().float()
    b = (cases.randn(f"depth.head{layers}.bias", 256) * 0.5).half().float()
    return w, b


def run(model, layers):
    """The recorded calls on a depther (the reference's or this package's), as name -> float32 array."""
    x = image()
    out = {}
    with torch.no_grad():
        out[f"L{layers}.whole"] = model.whole_inference(x, None, True)
        out[f"L{layers}.whole_raw"] = model.whole_inference(x, None, False)
        if layers == 4:
            out["L4.sized"] = model.whole_inference(x, [meta()] * 2, True, size=(17, 23))
            pair = model.aug_test([x, x.flip(3)], [[meta()] * 2, [meta(True)] * 2])
            out["L4.aug"] = torch.stack([torch.as_tensor(a) for a in pair])
            out["L4.slide"] = model.slide_inference(x, None, True, STRIDE, CROP)
            out["L4.simple"] = torch.stack([torch.as_tensor(a) for a in model.simple_test(x, [meta()] * 2)])
    return {k: v.float().cpu().numpy() for k, v in out.items()}
