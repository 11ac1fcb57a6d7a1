"""3-Augment of the DeiT-III recipe on the device, from uint8 batches.

The reference builds its training transform in ``deit/augment.py:90-123`` (``ThreeAugment=True``, ``color_jitter=0.3``):
``RandomResizedCropAndInterpolation``, ``RandomHorizontalFlip``, ``RandomChoice([gray_scale, Solarization, GaussianBlur])``,
``ColorJitter(j, j, j)``, ``ToTensor``, ``Normalize`` - per-sample PIL code in loader workers.  Here everything BEHIND THE CROP
runs as HIP kernels (csrc/augment.hip) on the decoded, cropped uint8 batch [B, H, W, 3]: a quarter of the bytes of the f32
batch on their way to the device, and no PIL chain on the host.  The kernels reproduce PIL's arithmetic bit for bit (the
contract is in include/octic_hip.h; tests/golden/augment_numpy.py restates it, tests/golden/augment.npz holds PIL's results).

THE CROP IN FRONT is ``octic_vits_amd/crop.py`` (csrc/crop.hip): ``ThreeAugment(crop=RandomResizedCrop())`` or, for ``--src``,
``crop=SrcCrop()`` takes the decoded sources of any sizes as a ``dino_augment.PackedImages``; ``apply_sources`` runs the crop launch
(uint8 crops of one size) and then the kernels of this module, and ``draw_sources`` draws, per sample, the crop's variates and
then the ones listed below - the reference pipeline's order on the shared ``random`` stream.  Without ``crop`` the input is the
uint8 HWC crops of one size that a host-side crop yields.  Decoding and the sampler (``RASampler``) stay on the host; hue jitter is
not part of this recipe.  The DINOv2 multi-crop augmentation is ``octic_vits_amd/dino_augment.py``.

``ThreeAugment.draw`` consumes the random streams exactly as the reference pipeline does for B samples in turn, per sample:

0. with ``crop`` (``draw_sources`` only): the crop's own draws, see ``octic_vits_amd/crop.py``;
1. flip: ``torch.rand(1) < hflip``;
2. ``RandomChoice``: one ``random.random()`` (``random.choices`` without weights: ``floor(random() * 3)``);
3. the chosen op's own ``random.random()`` test - at p = 1 always true, but consumed;
4. blur only: ``random.uniform(0.1, 2.0)``, the radius;
5. ``ColorJitter.get_params``: ``torch.randperm(4)`` (entry 3 is hue, which the recipe leaves ``None``: nothing is drawn or
   applied for it), then one ``torch.empty(1).uniform_(max(0, 1 - j), 1 + j)`` each for brightness, contrast, saturation;
6. ``color_jitter`` of ``None`` or 0: step 5 draws nothing and no jitter is applied.

``rng`` stands for the ``random`` module (default) or a ``random.Random``; ``generator`` for torch's global CPU generator
(default) or a ``torch.Generator``.
"""
import random
from dataclasses import dataclass

import numpy as np
import torch

from . import ops
from .mixup import TableUploader

__all__ = ["AugParams", "ThreeAugment", "AugTableUploader", "to_tensor", "blur_constants", "IMAGENET_DEFAULT_MEAN", "IMAGENET_DEFAULT_STD",
           "OP_NONE", "OP_GRAY", "OP_SOLARIZE", "OP_BLUR"]

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
OP_NONE, OP_GRAY, OP_SOLARIZE, OP_BLUR = 0, 1, 2, 3
_f32 = np.float32


def blur_constants(radius):
    """(r, ww, fw): the integer constants of one box pass of ``ImageFilter.GaussianBlur(radius)``.  PIL computes the box
    radius in C ``float``: every operation below rounds to float32 (in float64 the result is 1 ulp off at radii 0.9, 1.0 and
    1.3, and blurred pixels then differ by up to 2)."""
    rho = _f32(radius)
    s2 = _f32(_f32(rho * rho) / _f32(3))
    L = _f32(np.sqrt(_f32(_f32(_f32(12) * s2) + _f32(1))))
    l = _f32(np.floor(_f32(_f32(L - _f32(1)) / _f32(2))))
    a = _f32(_f32(_f32(_f32(2) * l) + _f32(1)) * _f32(_f32(l * _f32(l + _f32(1))) - _f32(_f32(3) * s2)))
    lp = _f32(l + _f32(1))
    a = _f32(a / _f32(_f32(6) * _f32(s2 - _f32(lp * lp))))
    fr = _f32(l + a)
    r = int(fr)
    ww = int(_f32(_f32(1 << 24) / _f32(_f32(fr * _f32(2)) + _f32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


@dataclass
class AugParams:
    """One draw for a batch of B samples: ``flip`` bool [B]; ``op`` int32 [B] (0 none, 1 grayscale, 2 solarize, 3 blur);
    ``radius`` float64 [B] (the blur radius, 0 elsewhere); ``order`` int32 [B, 4] (the jitter ops in application order: 0
    brightness, 1 contrast, 2 saturation, -1 skip); ``brightness``, ``contrast``, ``saturation`` float32 [B]."""
    flip: np.ndarray
    op: np.ndarray
    radius: np.ndarray
    order: np.ndarray
    brightness: np.ndarray
    contrast: np.ndarray
    saturation: np.ndarray

    def __post_init__(self):
        self.flip = np.ascontiguousarray(self.flip, dtype=bool)
        self.op = np.ascontiguousarray(self.op, dtype=np.int32)
        self.radius = np.ascontiguousarray(self.radius, dtype=np.float64)
        self.order = np.ascontiguousarray(self.order, dtype=np.int32).reshape(-1, 4)
        self.brightness = np.ascontiguousarray(self.brightness, dtype=np.float32)
        self.contrast = np.ascontiguousarray(self.contrast, dtype=np.float32)
        self.saturation = np.ascontiguousarray(self.saturation, dtype=np.float32)
        B = self.flip.shape[0]
        if self.order.shape != (B, 4) or any(getattr(self, n).shape != (B,) for n in self._VECTORS):
            raise ValueError("AugParams: flip, op, radius and the three factors must be [B] and order [B, 4]")

    _VECTORS = ("flip", "op", "radius", "brightness", "contrast", "saturation")

    @classmethod
    def identity(cls, B):
        """Nothing but ToTensor + Normalize."""
        one = np.ones(B, np.float32)
        return cls(np.zeros(B, bool), np.zeros(B, np.int32), np.zeros(B), np.full((B, 4), -1, np.int32), one, one.copy(), one.copy())

    def __len__(self):
        return int(self.flip.shape[0])

    def __eq__(self, other):
        return isinstance(other, AugParams) and np.array_equal(self.order, other.order) and all(
            np.array_equal(getattr(self, n), getattr(other, n)) for n in self._VECTORS)

    def table(self):
        """The packed rows the kernels read (``octic_aug_row``, include/octic_hip.h): int32 [B, 16] =
        flip | op | blur r | blur ww | blur fw | order[4] | brightness, contrast, saturation (f32 bits) | 0 0 0 0."""
        B = len(self)
        if ((self.op < 0) | (self.op > 3)).any():
            raise ValueError("AugParams: op must be 0 (none), 1 (grayscale), 2 (solarize) or 3 (blur)")
        t = np.zeros((B, 16), dtype=np.int32)
        t[:, 0] = self.flip
        t[:, 1] = self.op
        for i in np.nonzero(self.op == OP_BLUR)[0]:
            if not 0.0 < self.radius[i] <= 2.0:
                raise ValueError(f"AugParams: blur radius {self.radius[i]} outside (0, 2] (the kernels keep a 6-pixel halo)")
            t[i, 2:5] = blur_constants(self.radius[i])
        t[:, 5:9] = np.where((self.order >= 0) & (self.order <= 2), self.order, -1)
        t[:, 9] = self.brightness.view(np.int32)
        t[:, 10] = self.contrast.view(np.int32)
        t[:, 11] = self.saturation.view(np.int32)
        return t


class AugTableUploader(TableUploader):
    """``mixup.TableUploader`` for the 16-word rows of ``AugParams.table()``."""

    def __init__(self, B, device, slots=4):
        self.table = torch.from_numpy(AugParams.identity(B).table()).to(device)
        self._ring = [[torch.empty(B, 16, dtype=torch.int32).pin_memory(), None] for _ in range(slots)]
        self._i = 0


class ThreeAugment:
    """The reference's 3-Augment behind the crop on the HIP kernels of csrc/augment.hip (see the module docstring for the
    draw order).  ``apply`` maps a uint8 [B, H, W, 3] batch on the GPU to the normalised f32 [B, 3, H, W] batch."""

    def __init__(self, color_jitter=0.3, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, hflip=0.5, rng=None, generator=None,
                 crop=None):
        if color_jitter is not None and color_jitter < 0:
            raise ValueError("ThreeAugment: color_jitter must be non-negative")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("ThreeAugment: mean and std take three values each")
        self.color_jitter = color_jitter
        # Normalize(mean=torch.tensor(mean), std=torch.tensor(std)): rounded to f32 once
        self.mean = tuple(float(_f32(v)) for v in mean)
        self.std = tuple(float(_f32(v)) for v in std)
        self.hflip = hflip
        self.rng = random if rng is None else rng
        self.generator = generator
        if crop is not None and not (hasattr(crop, "draw_one") and hasattr(crop, "launch")):
            raise TypeError(f"ThreeAugment: `crop` must be a transform of octic_vits_amd.crop, got {type(crop).__name__}")
        self.crop = crop
        self._workspaces = {}

    # ---- the host side -------------------------------------------------------------------------------------------------
    def draw(self, B):
        """One draw for B samples, sample by sample in the reference pipeline's order."""
        p = AugParams.identity(int(B))
        for i in range(len(p)):
            self._draw_sample(p, i)
        return p

    def _draw_sample(self, p, i):
        r, g = self.rng, self.generator
        p.flip[i] = bool(torch.rand(1, generator=g) < self.hflip)
        choice = int(r.random() * 3)
        if choice == 2:
            if r.random() <= 1.0:
                p.op[i] = OP_BLUR
                p.radius[i] = r.uniform(0.1, 2.0)
        elif r.random() < 1.0:
            p.op[i] = OP_GRAY if choice == 0 else OP_SOLARIZE
        if self.color_jitter is not None and not self.color_jitter == 0:
            lo, hi = max(0.0, 1.0 - self.color_jitter), 1.0 + self.color_jitter
            perm = torch.randperm(4, generator=g).numpy()
            p.order[i] = np.where(perm < 3, perm, -1)
            p.brightness[i] = float(torch.empty(1).uniform_(lo, hi, generator=g))
            p.contrast[i] = float(torch.empty(1).uniform_(lo, hi, generator=g))
            p.saturation[i] = float(torch.empty(1).uniform_(lo, hi, generator=g))

    def _need_crop(self, what):
        if self.crop is None:
            raise RuntimeError(f"ThreeAugment.{what}: built without `crop` (octic_vits_amd.crop.RandomResizedCrop or SrcCrop)")

    def draw_sources(self, heights, widths):
        """One draw for B decoded sources of the given sizes -> (``CropParams``, ``AugParams``): per sample, in turn, the crop's
        draws and then what ``draw`` consumes for that sample - the reference pipeline's stream order."""
        self._need_crop("draw_sources")
        heights = np.ascontiguousarray(heights, dtype=np.int64).reshape(-1)
        widths = np.ascontiguousarray(widths, dtype=np.int64).reshape(-1)
        if heights.shape != widths.shape or len(heights) == 0 or min(heights.min(), widths.min()) < 1:
            raise ValueError("ThreeAugment.draw_sources: heights and widths must be [B] each, B >= 1, all sides >= 1")
        p, drawn = AugParams.identity(len(heights)), []
        for i in range(len(p)):
            drawn.append(self.crop.draw_one(int(heights[i]), int(widths[i])))
            self._draw_sample(p, i)
        return self.crop.params(heights, widths, drawn), p

    # ---- the device side -----------------------------------------------------------------------------------------------
    @staticmethod
    def check_batch(images_u8, what="ThreeAugment"):
        if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[3] != 3:
            got = f"{tuple(images_u8.shape)} {images_u8.dtype}" if torch.is_tensor(images_u8) else type(images_u8).__name__
            raise TypeError(f"{what}: images must be a uint8 [B, H, W, 3] batch (decoded, cropped, HWC), got {got}")
        ops._require_cuda(images_u8)

    def _workspace(self, B, H, W, device):
        key = (B, H, W, str(device))
        ws = self._workspaces.get(key)
        if ws is None:
            ws = self._workspaces[key] = ops.augment_workspace(B, H, W, device)
        return ws

    def launch(self, images_u8, table, out=None, uint8_out=False):
        """The launches alone, for a table that is already on the device (what a captured step records)."""
        self.check_batch(images_u8)
        B, H, W, _ = images_u8.shape
        if out is None:
            out = (torch.empty(B, H, W, 3, dtype=torch.uint8, device=images_u8.device) if uint8_out else
                   torch.empty(B, 3, H, W, dtype=torch.float32, device=images_u8.device))
        elif (out.dtype == torch.uint8) != bool(uint8_out):
            raise TypeError("ThreeAugment: `out` is uint8 with uint8_out=True, float32 otherwise")
        return ops.augment_u8(images_u8.contiguous(), table, self.mean, self.std, out, self._workspace(B, H, W, images_u8.device))

    def apply(self, images_u8, params=None, out=None, uint8_out=False):
        """The augmented batch: f32 [B, 3, H, W], normalised (the model's input), or with ``uint8_out`` the uint8 [B, H, W, 3]
        pixels in front of ``ToTensor``.  params: an ``AugParams`` (default: a fresh ``draw``); out: the output buffer (must
        not overlap the input).  The input is left untouched."""
        self.check_batch(images_u8)
        B = images_u8.shape[0]
        if params is None:
            params = self.draw(B)
        elif len(params) != B:
            raise ValueError("ThreeAugment.apply: the parameters were drawn for another batch size")
        table = torch.from_numpy(params.table()).to(images_u8.device)
        return self.launch(images_u8, table, out=out, uint8_out=uint8_out)

    def apply_sources(self, packed, params=None, out=None, uint8_out=False):
        """``apply`` for a ``dino_augment.PackedImages`` of decoded sources: the crop launch (uint8 crops), then the launches of
        ``apply``.  params: the pair ``draw_sources`` returns (default: a fresh one)."""
        self._need_crop("apply_sources")
        from .dino_augment import PackedImages
        if not isinstance(packed, PackedImages):
            raise TypeError(f"ThreeAugment.apply_sources: `packed` must be a PackedImages (pack_images), got {type(packed).__name__}")
        if params is None:
            params = self.draw_sources(*packed.host_sizes())
        crop_params, aug_params = params
        return self.apply(self.crop.apply(packed, crop_params, uint8_out=True), aug_params, out=out, uint8_out=uint8_out)

    def to_tensor(self, images_u8, out=None):
        """``ToTensor`` + ``Normalize`` only (the identity row): the evaluation loader's transform behind its crop."""
        self.check_batch(images_u8)
        return self.apply(images_u8, AugParams.identity(images_u8.shape[0]), out=out)

    def __call__(self, images_u8):
        return self.apply(images_u8)


_DEFAULT = None


def to_tensor(images_u8, out=None):
    """``ToTensor`` + ``Normalize`` with ImageNet's mean / std for a uint8 [B, H, W, 3] batch on the GPU -> f32 [B, 3, H, W]."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = ThreeAugment()
    return _DEFAULT.to_tensor(images_u8, out=out)
