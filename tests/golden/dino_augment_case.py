"""The oracle of the DINOv2 multi-crop augmentation tests: ``DataAugmentationDINO`` (dinov2/data/augmentations.py with the
``GaussianBlur`` of dinov2/data/transforms.py) for ONE PIL image, in front of ``ToTensor`` + ``Normalize``, and the order in
which it consumes torch's generator.  Every pixel operation on a PIL image is the real PIL call; the torchvision glue
(``RandomResizedCrop.get_params``, ``ColorJitter``, ``adjust_hue``, ``RandomGrayscale``, ``GaussianBlur`` - which works on a
float32 tensor -, ``RandomSolarize``, ``RandomApply``) is restated from its published algorithm: torchvision is not installed
here.  PIL is imported lazily: the draw needs none.

One crop's parameters: a dict with ``box`` (top, left, h, w), ``size``, ``flip``, ``jitter``, ``order`` (0 brightness,
1 contrast, 2 saturation, 3 hue), ``brightness``, ``contrast``, ``saturation``, ``hue``, ``gray``, ``blur``, ``sigma``,
``solarize``."""
import math

import numpy as np
import torch

FIELDS = ("box", "size", "flip", "jitter", "order", "brightness", "contrast", "saturation", "hue", "gray", "blur", "sigma",
          "solarize")
RATIO = (3.0 / 4.0, 4.0 / 3.0)


def identity(box, size):
    return dict(box=tuple(int(v) for v in box), size=int(size), flip=False, jitter=False, order=[0, 1, 2, 3], brightness=1.0,
                contrast=1.0, saturation=1.0, hue=0.0, gray=False, blur=False, sigma=0.0, solarize=False)


# ------------------------------------------------------------------------------------------------ pixels
def adjust_hue_pil(img, hue_factor):
    from PIL import Image
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h = np_h + np.array(int(hue_factor * 255)).astype(np.uint8)      # uint8 arithmetic: wraps
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def gaussian_blur_pil(img, sigma):
    """F.gaussian_blur(pil, [9, 9], [sigma, sigma]): uint8 tensor -> float32, reflect pad 4, conv2d with k (x) k, round, uint8."""
    from PIL import Image
    x = torch.linspace(-4.0, 4.0, steps=9, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = pdf / pdf.sum()
    k2 = torch.mm(k1[:, None], k1[None, :])
    t = torch.from_numpy(np.asarray(img).copy()).permute(2, 0, 1)[None].to(torch.float32)
    t = torch.nn.functional.pad(t, [4, 4, 4, 4], mode="reflect")
    t = torch.nn.functional.conv2d(t, k2.expand(3, 1, 9, 9), groups=3)
    t = torch.round(t).to(torch.uint8)[0].permute(1, 2, 0).contiguous()
    return Image.fromarray(t.numpy(), "RGB")


def color_chain_pil(img, p):
    from PIL import Image, ImageEnhance, ImageOps
    if p["jitter"]:
        for fn in p["order"]:
            if fn == 0:
                img = ImageEnhance.Brightness(img).enhance(float(p["brightness"]))
            elif fn == 1:
                img = ImageEnhance.Contrast(img).enhance(float(p["contrast"]))
            elif fn == 2:
                img = ImageEnhance.Color(img).enhance(float(p["saturation"]))
            elif fn == 3:
                img = adjust_hue_pil(img, float(p["hue"]))
    if p["gray"]:
        g = img.convert("L")
        img = Image.merge("RGB", (g, g, g))
    if p["blur"]:
        img = gaussian_blur_pil(img, float(p["sigma"]))
    if p["solarize"]:
        img = ImageOps.solarize(img, 128)
    return img


def apply_pil(img, p):
    from PIL import Image
    top, left, h, w = p["box"]
    img = img.crop((left, top, left + w, top + h)).resize((p["size"], p["size"]), Image.BICUBIC)
    if p["flip"]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return color_chain_pil(img, p)


def _img(px):
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(px, dtype=np.uint8), "RGB")


def apply_u8(src, p):
    """uint8 source [H, W, 3] -> the crop in front of ToTensor, uint8 [S, S, 3], through PIL."""
    return np.asarray(apply_pil(_img(src), p)).copy()


def color_chain_u8(crop, p):
    return np.asarray(color_chain_pil(_img(crop), p)).copy()


# ------------------------------------------------------------------------------------------------ the draw
def _uniform(lo, hi, g):
    return torch.empty(1).uniform_(lo, hi, generator=g).item()


def get_crop_params(height, width, scale, g):
    """RandomResizedCrop.get_params with ratio (3/4, 4/3)."""
    area = height * width
    log_ratio = torch.log(torch.tensor(RATIO))
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], g)
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1], generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(RATIO):
        w = width
        h = int(round(w / min(RATIO)))
    elif in_ratio > max(RATIO):
        h = height
        w = int(round(h * max(RATIO)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def draw_crop(height, width, scale, size, blur_p, may_solarize, g):
    """One crop: geometry, flip, RandomApply(ColorJitter, 0.8), RandomGrayscale(0.2), the reference's GaussianBlur(p=blur_p)
    (which hands RandomApply 1 - blur_p, and RandomApply skips when ITS p < rand), RandomSolarize(0.2) for global 2."""
    p = identity(get_crop_params(height, width, scale, g), size)
    p["flip"] = bool(torch.rand(1, generator=g) < 0.5)
    if not 0.8 < torch.rand(1, generator=g):
        p["jitter"] = True
        p["order"] = [int(v) for v in torch.randperm(4, generator=g)]
        p["brightness"] = _uniform(0.6, 1.4, g)
        p["contrast"] = _uniform(0.6, 1.4, g)
        p["saturation"] = _uniform(0.8, 1.2, g)
        p["hue"] = _uniform(-0.1, 0.1, g)
    p["gray"] = bool(torch.rand(1, generator=g) < 0.2)
    keep_p = 1 - blur_p
    if not keep_p < torch.rand(1, generator=g):
        p["blur"] = True
        p["sigma"] = _uniform(0.1, 2.0, g)
    if may_solarize:
        p["solarize"] = bool(torch.rand(1, generator=g) < 0.2)
    return p


def draw_image(height, width, generator=None, global_crops_scale=(0.32, 1.0), local_crops_scale=(0.05, 0.32),
               local_crops_number=8, global_crops_size=224, local_crops_size=96):
    """The 2 + n crops of one image in the reference's order: global 1, global 2, local 1..n."""
    g = generator
    out = [draw_crop(height, width, global_crops_scale, global_crops_size, 1.0, False, g),
           draw_crop(height, width, global_crops_scale, global_crops_size, 0.1, True, g)]
    for _ in range(local_crops_number):
        out.append(draw_crop(height, width, local_crops_scale, local_crops_size, 0.5, False, g))
    return out


# ------------------------------------------------------------------------------------------------ storage
def pack(crops):
    """A list of parameter dicts -> arrays for an npz file."""
    out = {}
    for f in FIELDS:
        dt = {"box": np.int32, "size": np.int32, "order": np.int32, "flip": bool, "jitter": bool, "gray": bool, "blur": bool,
              "solarize": bool}.get(f, np.float64)
        out[f] = np.array([c[f] for c in crops], dtype=dt)
    return out


def unpack(arrays, prefix=""):
    n = len(arrays[prefix + "size"])
    out = []
    for i in range(n):
        p = {}
        for f in FIELDS:
            v = arrays[prefix + f][i]
            p[f] = [int(x) for x in v] if f in ("box", "order") else (int(v) if f == "size" else (
                float(v) if f in ("brightness", "contrast", "saturation", "hue", "sigma") else bool(v)))
        p["box"] = tuple(p["box"])
        out.append(p)
    return out
