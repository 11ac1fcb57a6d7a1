"""The oracle of the 3-Augment tests: the DeiT-III training transform behind the crop (horizontal flip, one of grayscale /
solarize / Gaussian blur, ColorJitter, before ToTensor + Normalize) for ONE PIL image and ONE parameter set, and the order in
which that pipeline consumes its random streams.  Every pixel operation is the real PIL call; only the torchvision glue
(``Grayscale(3)``, ``ColorJitter``'s order and factors, ``RandomChoice``) is restated, from the published algorithm -
torchvision and timm are not installed here.  PIL is imported lazily: the draw order needs none.

Parameters of one sample (``params``): a dict with ``flip`` (bool), ``op`` (0 none, 1 grayscale, 2 solarize, 3 blur),
``radius`` (float, blur only), ``order`` (the jitter ops in application order: 0 brightness, 1 contrast, 2 saturation; anything
else, e.g. 3 = hue or -1, is skipped) and the factors ``brightness``, ``contrast``, ``saturation`` (floats)."""
import random

import numpy as np
import torch

OP_NONE, OP_GRAY, OP_SOLARIZE, OP_BLUR = 0, 1, 2, 3


def apply_pil(img, params):
    """The augmented PIL RGB image."""
    from PIL import Image, ImageEnhance, ImageFilter, ImageOps
    if params["flip"]:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)          # RandomHorizontalFlip -> F.hflip
    op = int(params["op"])
    if op == OP_GRAY:                                       # Grayscale(3): convert("L"), the band three times
        g = img.convert("L")
        img = Image.merge("RGB", (g, g, g))
    elif op == OP_SOLARIZE:
        img = ImageOps.solarize(img)
    elif op == OP_BLUR:
        img = img.filter(ImageFilter.GaussianBlur(radius=float(params["radius"])))
    for fn in params["order"]:                              # ColorJitter.forward: adjust_* = ImageEnhance.*(img).enhance(f)
        if fn == 0:
            img = ImageEnhance.Brightness(img).enhance(float(params["brightness"]))
        elif fn == 1:
            img = ImageEnhance.Contrast(img).enhance(float(params["contrast"]))
        elif fn == 2:
            img = ImageEnhance.Color(img).enhance(float(params["saturation"]))
    return img


def apply_u8(pixels, params):
    """uint8 [H, W, 3] -> the augmented uint8 [H, W, 3] through PIL."""
    from PIL import Image
    return np.asarray(apply_pil(Image.fromarray(np.ascontiguousarray(pixels), "RGB"), params)).copy()


def draw_sample(color_jitter=0.3, hflip=0.5, rng=random, generator=None):
    """The parameters of one sample, drawn as the reference pipeline draws them: ``torch.rand(1) < hflip``
    (RandomHorizontalFlip); one ``random.random()`` for ``RandomChoice`` (``random.choices`` without weights:
    ``floor(random() * 3)``); the chosen op's own ``random.random()`` test at p = 1; ``random.uniform(0.1, 2.0)`` for the blur;
    then ColorJitter.get_params: ``torch.randperm(4)`` and one ``torch.empty(1).uniform_(lo, hi)`` each for brightness,
    contrast and saturation (hue is None in the recipe: no draw, its slot in the permutation does nothing)."""
    p = dict(flip=False, op=OP_NONE, radius=0.0, order=[-1, -1, -1, -1], brightness=1.0, contrast=1.0, saturation=1.0)
    p["flip"] = bool(torch.rand(1, generator=generator) < hflip)
    choice = int(rng.random() * 3)
    if choice == 0:
        p["op"] = OP_GRAY if rng.random() < 1.0 else OP_NONE
    elif choice == 1:
        p["op"] = OP_SOLARIZE if rng.random() < 1.0 else OP_NONE
    else:
        if rng.random() <= 1.0:
            p["op"] = OP_BLUR
            p["radius"] = rng.uniform(0.1, 2.0)
    if color_jitter is not None and not color_jitter == 0:
        lo, hi = max(0.0, 1.0 - color_jitter), 1.0 + color_jitter
        p["order"] = [int(v) if int(v) < 3 else -1 for v in torch.randperm(4, generator=generator)]
        for name in ("brightness", "contrast", "saturation"):
            p[name] = float(torch.empty(1).uniform_(lo, hi, generator=generator))
    return p
