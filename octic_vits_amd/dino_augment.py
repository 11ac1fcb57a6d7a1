"""DINOv2's multi-crop augmentation on the device, from a ragged batch of decoded uint8 images.

The reference's ``DataAugmentationDINO`` (``dinov2/data/augmentations.py``, with the ``GaussianBlur`` of
``dinov2/data/transforms.py``) makes 2 global and ``local_crops_number`` local crops per image in PIL / torchvision code on
loader workers: bicubic ``RandomResizedCrop``, ``RandomHorizontalFlip``, ``RandomApply(ColorJitter(0.4, 0.4, 0.2, 0.1), 0.8)``,
``RandomGrayscale(0.2)``, a 9 x 9 ``GaussianBlur``, ``RandomSolarize`` (global 2 only), ``ToTensor``, ``Normalize``.  Here the
decoded sources go to the device as they are (``pack_images``: uint8, back to back, any sizes) and everything behind the
decoder runs as HIP kernels (csrc/dino_augment.hip).  The kernels reproduce Pillow's arithmetic bit for bit and torchvision's
blur up to its rounding ties (the contract is in include/octic_hip.h; tests/golden/dino_augment_numpy.py restates it,
tests/golden/dino_augment.npz holds PIL's results).  ``DinoAugment.collate`` returns the dictionary ``ssl.SSLTrainer.step``
takes.

THE DRAW stays on the host and consumes torch's generator exactly as the reference does, image by image and, per image, for
global 1, global 2, local 1..n in turn:

1. ``RandomResizedCrop.get_params``: up to 10 tries of ``uniform_(scale)`` (area) and ``exp(uniform_(log 3/4, log 4/3))``
   (aspect); a try that fits draws ``randint(0, H - h + 1)`` and ``randint(0, W - w + 1)``; else the central-crop fallback;
2. flip: ``torch.rand(1) < 0.5``;
3. ``RandomApply(ColorJitter, p=0.8)``: one ``torch.rand(1)``, skipped when ``0.8 < rand``; if applied ``torch.randperm(4)``
   and one ``uniform_`` each for brightness [0.6, 1.4], contrast [0.6, 1.4], saturation [0.8, 1.2], hue [-0.1, 0.1];
4. grayscale: ``torch.rand(1) < 0.2``;
5. blur: the reference's ``GaussianBlur(p)`` hands ``RandomApply`` 1 - p, and ``RandomApply`` skips when ITS p < rand: global 1
   (p = 1.0) is blurred only when rand == 0, global 2 (p = 0.1) when rand <= 0.9, the locals (p = 0.5) when rand <= 0.5 -
   reproduced as shipped; if blurred ``uniform_(0.1, 2.0)`` for sigma;
6. global 2 only: solarize when ``torch.rand(1) < 0.2``.

The host also computes the integer resampling coefficients of every crop (Pillow's ``precompute_coeffs`` in float64); the
kernels do integer sums only.  Not built: decoding, the sampler, tensor-mode or antialiased torchvision resizing.
"""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from . import ops
from . import ssl as _ssl
from .augment import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD

__all__ = ["PackedImages", "pack_images", "DinoAugParams", "DinoAugment", "resize_coeffs", "blur_weights", "hue_shift",
           "upload_tables", "ROW_WORDS"]

ROW_WORDS = ops.DINO_ROW_WORDS
_f32 = np.float32
_RATIO = (3.0 / 4.0, 4.0 / 3.0)
_POOL_MAX = (1 << 31) - 1


# ------------------------------------------------------------------------------------------------ the ragged batch
@dataclass
class PackedImages:
    """Decoded images of different sizes on the device: ``data`` uint8 1-D (the [H_i, W_i, 3] images back to back), ``offsets``
    int64 [B] (bytes), ``heights`` / ``widths`` int32 [B].  ``sizes`` keeps (heights, widths) on the host for the draw."""
    data: torch.Tensor
    offsets: torch.Tensor
    heights: torch.Tensor
    widths: torch.Tensor
    sizes: tuple = None

    def __len__(self):
        return int(self.offsets.shape[0])

    def host_sizes(self):
        if self.sizes is None:
            self.sizes = (self.heights.cpu().numpy().astype(np.int64), self.widths.cpu().numpy().astype(np.int64))
        return self.sizes


def _require_gpu(t, what):
    if not t.is_cuda:
        raise TypeError(f"{what} must be on the GPU (the augmentation has no CPU path), got a CPU tensor")


def pack_images(images, device):
    """A list of decoded uint8 [H_i, W_i, 3] arrays or tensors of any sizes -> ``PackedImages`` on ``device``: one host
    buffer, one upload."""
    device = torch.device(device)
    if device.type != "cuda":
        raise TypeError(f"pack_images: `device` must be a GPU (the augmentation has no CPU path), got {device}")
    if len(images) == 0:
        raise ValueError("pack_images: `images` is empty")
    flat, hs, ws = [], [], []
    for i, im in enumerate(images):
        t = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
        if t.dtype != torch.uint8:
            raise TypeError(f"pack_images: images[{i}] must be uint8 (decoded pixels), got {t.dtype}")
        if t.dim() != 3 or t.shape[2] != 3:
            raise ValueError(f"pack_images: images[{i}] must be [H, W, 3], got {tuple(t.shape)}")
        if t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"pack_images: images[{i}] has a side below 1: {tuple(t.shape)}")
        flat.append(t.cpu().contiguous().reshape(-1))
        hs.append(int(t.shape[0]))
        ws.append(int(t.shape[1]))
    hs, ws = np.asarray(hs, np.int64), np.asarray(ws, np.int64)
    nbytes = hs * ws * 3
    offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).astype(np.int64)
    host = torch.empty(int(nbytes.sum()), dtype=torch.uint8).pin_memory()
    torch.cat(flat, out=host)
    return PackedImages(host.to(device, non_blocking=True), torch.from_numpy(offsets).to(device),
                        torch.from_numpy(hs.astype(np.int32)).to(device), torch.from_numpy(ws.astype(np.int32)).to(device),
                        (hs, ws))


# ------------------------------------------------------------------------------------------------ host arithmetic
def resize_taps(n, S):
    """Taps per output pixel of Pillow's bicubic resample n -> S (1 for the skipped pass)."""
    return 1 if n == S else int(math.ceil(2.0 * max(n / S, 1.0))) * 2 + 1


def max_resize_taps(max_side, S):
    """The most taps any crop length 1 <= n <= max_side needs at output size S >= 5.  ``resize_taps`` grows with n except at
    n == S, where the pass is skipped (1 tap), and every n < S needs 5: so max_side == S is bounded by its neighbours."""
    return max(resize_taps(max_side, S), 5)


@lru_cache(maxsize=4096)
def resize_coeffs(n, S):
    """Pillow's 8-bit bicubic coefficients for one axis, crop length n -> S: (bounds int32 [S, 2] = (xmin, count), k int32
    [S, taps]), float64 as ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` (host code of the library:
    ``octic_dino_resize_coeffs``); n == S (Pillow skips the pass) is one tap of 2^22.  The arrays are cached: do not write them."""
    n, S = int(n), int(S)
    if n < 1 or S < 1:
        raise ValueError(f"resize_coeffs: lengths must be positive, got {n} -> {S}")
    return ops.dino_resize_coeffs(n, S, resize_taps(n, S))


def blur_weights(sigma):
    """The nine f32 weights of torchvision's ``_get_gaussian_kernel1d(9, sigma)``, computed with torch as it does."""
    x = torch.linspace(-4.0, 4.0, steps=9, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    return (pdf / pdf.sum()).numpy()


def hue_shift(hue_factor):
    """torchvision's uint8 addend to H: ``(uint8)(int)(hue_factor 255)``, truncated toward zero, wrapped mod 256."""
    return int(float(hue_factor) * 255) % 256


def _uniform(lo, hi, g):
    return torch.empty(1).uniform_(lo, hi, generator=g).item()


_LOG_RATIO = None


def _crop_box(height, width, scale, g):
    """``RandomResizedCrop.get_params`` (ratio 3/4 .. 4/3): (top, left, h, w)."""
    global _LOG_RATIO
    if _LOG_RATIO is None:
        _LOG_RATIO = torch.log(torch.tensor(_RATIO))
    area = height * width
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], g)
        aspect_ratio = torch.exp(torch.empty(1).uniform_(_LOG_RATIO[0], _LOG_RATIO[1], generator=g)).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = torch.randint(0, height - h + 1, size=(1,), generator=g).item()
            j = torch.randint(0, width - w + 1, size=(1,), generator=g).item()
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(_RATIO):
        w = width
        h = int(round(w / min(_RATIO)))
    elif in_ratio > max(_RATIO):
        h = height
        w = int(round(h * max(_RATIO)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


# ------------------------------------------------------------------------------------------------ one draw
class DinoAugParams:
    """Everything random about one batch of B images with C = 2 + n_local crops each, as numpy arrays, CROP-MAJOR (index
    [c, b]: crop c of image b; c = 0, 1 are the globals): ``box`` int32 [C, B, 4] (top, left, h, w), ``flip`` bool [C, B],
    ``jitter`` bool [C, B], ``order`` int32 [C, B, 4] (0 brightness, 1 contrast, 2 saturation, 3 hue), ``brightness``,
    ``contrast``, ``saturation`` float32 [C, B], ``hue`` float64 [C, B], ``gray``, ``blur``, ``solarize`` bool [C, B], ``sigma``
    float64 [C, B]; with the batch's ``heights`` / ``widths`` int64 [B] and the two output sizes."""
    _FIELDS = (("box", np.int32, (4,)), ("flip", bool, ()), ("jitter", bool, ()), ("order", np.int32, (4,)),
               ("brightness", np.float32, ()), ("contrast", np.float32, ()), ("saturation", np.float32, ()), ("hue", np.float64, ()),
               ("gray", bool, ()), ("blur", bool, ()), ("sigma", np.float64, ()), ("solarize", bool, ()))

    def __init__(self, heights, widths, n_local, global_size, local_size, **arrays):
        self.heights = np.ascontiguousarray(heights, dtype=np.int64).reshape(-1)
        self.widths = np.ascontiguousarray(widths, dtype=np.int64).reshape(-1)
        if self.heights.shape != self.widths.shape:
            raise ValueError("DinoAugParams: heights and widths must be [B] each")
        self.n_local, self.global_size, self.local_size = int(n_local), int(global_size), int(local_size)
        C, B = 2 + self.n_local, len(self.heights)
        for name, dt, tail in self._FIELDS:
            if name in arrays:
                v = np.ascontiguousarray(arrays.pop(name), dtype=dt)
                if v.shape != (C, B) + tail:
                    raise ValueError(f"DinoAugParams: {name} must be {(C, B) + tail} (crop-major), got {v.shape}")
            else:
                v = np.zeros((C, B) + tail, dt)
                if name in ("brightness", "contrast", "saturation"):
                    v += 1
                if name == "order":
                    v[...] = np.arange(4)
            setattr(self, name, v)
        if arrays:
            raise TypeError(f"DinoAugParams: unknown fields {sorted(arrays)}")

    def __len__(self):
        return len(self.heights)

    @property
    def n_crops(self):
        return 2 + self.n_local

    def __eq__(self, other):
        return (isinstance(other, DinoAugParams) and np.array_equal(self.heights, other.heights) and
                np.array_equal(self.widths, other.widths) and
                (self.n_local, self.global_size, self.local_size) == (other.n_local, other.global_size, other.local_size) and
                all(np.array_equal(getattr(self, n), getattr(other, n)) for n, _, _ in self._FIELDS))

    def crop(self, c, b):
        """Crop c of image b as the parameter dict of tests/golden/dino_augment_case.py."""
        return dict(box=tuple(int(v) for v in self.box[c, b]), size=self.global_size if c < 2 else self.local_size,
                    flip=bool(self.flip[c, b]), jitter=bool(self.jitter[c, b]), order=[int(v) for v in self.order[c, b]],
                    brightness=float(self.brightness[c, b]), contrast=float(self.contrast[c, b]),
                    saturation=float(self.saturation[c, b]), hue=float(self.hue[c, b]), gray=bool(self.gray[c, b]),
                    blur=bool(self.blur[c, b]), sigma=float(self.sigma[c, b]), solarize=bool(self.solarize[c, b]))

    def color_rows(self, crops):
        """int32 [len(crops), ROW_WORDS]: the rows of the given (c, b) pairs with the fields behind the resize only."""
        t = np.zeros((len(crops), ROW_WORDS), np.int32)
        for i, (c, b) in enumerate(crops):
            t[i, 13:17] = np.where((self.order[c, b] >= 0) & (self.order[c, b] <= 3), self.order[c, b], -1) if self.jitter[c, b] else -1
            t[i, 17:20] = np.array([self.brightness[c, b], self.contrast[c, b], self.saturation[c, b]], _f32).view(np.int32)
            t[i, 20] = hue_shift(self.hue[c, b])
            t[i, 21], t[i, 22], t[i, 23] = self.gray[c, b], self.blur[c, b], self.solarize[c, b]
            if self.blur[c, b]:
                if not self.sigma[c, b] > 0:
                    raise ValueError(f"DinoAugParams: sigma must be positive, got {self.sigma[c, b]}")
                t[i, 24:33] = blur_weights(self.sigma[c, b]).view(np.int32)
        return t

    def tables(self):
        """What the kernels read (``octic_dino_row`` and the coefficient pool, include/octic_hip.h), packed on the host:
        ``rows_global`` int32 [2 B, ROW_WORDS], ``rows_local`` int32 [n_local B, ROW_WORDS] (crop-major) and ``coef`` int32
        1-D.  Row words: src_offset (2) | src_h src_w | top left h w | flip | hcoef htaps vcoef vtaps | order[4] |
        brightness contrast saturation (f32 bits) | hue_shift | gray blur solarize | blur_w[9] (f32 bits) | 0 x 7."""
        B, C = len(self), self.n_crops
        offsets = np.concatenate([[0], np.cumsum(self.heights * self.widths * 3)[:-1]]).astype(np.int64)
        pairs = [(c, b) for c in range(C) for b in range(B)]
        rows = self.color_rows(pairs)
        pool, at = [], 0
        for i, (c, b) in enumerate(pairs):
            S = self.global_size if c < 2 else self.local_size
            top, left, h, w = (int(v) for v in self.box[c, b])
            if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= self.heights[b] and left + w <= self.widths[b]):
                raise ValueError(f"DinoAugParams: box {(top, left, h, w)} of crop {c}, image {b} leaves its {self.heights[b]} x {self.widths[b]} source")
            rows[i, 0:2] = np.array([offsets[b]], np.int64).view(np.int32)
            rows[i, 2:9] = (self.heights[b], self.widths[b], top, left, h, w, self.flip[c, b])
            for word, n in ((9, w), (11, h)):
                bounds, k = resize_coeffs(n, S)
                if at + bounds.size + k.size > _POOL_MAX:
                    raise ValueError(f"DinoAugParams: the coefficient pool of this batch exceeds {_POOL_MAX} int32 words (the rows hold "
                                     "32-bit offsets); use a smaller batch")
                rows[i, word], rows[i, word + 1] = at, k.shape[1]
                pool += [bounds.reshape(-1), k.reshape(-1)]
                at += bounds.size + k.size
        coef = np.concatenate(pool) if pool else np.zeros(0, np.int32)
        return {"rows_global": np.ascontiguousarray(rows[:2 * B]), "rows_local": np.ascontiguousarray(rows[2 * B:]),
                "coef": np.ascontiguousarray(coef, dtype=np.int32)}


# ------------------------------------------------------------------------------------------------ the transform
def upload_tables(dev, tables, uploaded, device):
    """Host tables (numpy, by name) -> the device tables ``dev`` = {name: (device tensor, pinned staging)} through their staging
    buffers; only the used part of each travels.  ``uploaded`` keeps the event of the last upload per table set: the staging
    buffers are reused only when it has passed."""
    done = uploaded.get(id(dev))
    if done is not None:
        done.synchronize()                                  # the staging buffers are free again
    out = {}
    for k, (d, pinned) in dev.items():
        src = torch.from_numpy(tables[k])
        n = src.shape[0]
        pinned[:n].copy_(src)
        d[:n].copy_(pinned[:n], non_blocking=True)
        out[k] = d
    done = uploaded[id(dev)] = torch.cuda.Event()
    done.record(torch.cuda.current_stream(device))
    return out


class DinoAugment:
    """``DataAugmentationDINO`` on the HIP kernels of csrc/dino_augment.hip; the defaults are ``ssl_default_config.yaml``'s.
    ``max_side`` bounds the sources' sides (the loader's job): it fixes the capacity of the device tables."""

    def __init__(self, global_crops_scale=(0.32, 1.0), local_crops_scale=(0.05, 0.32), local_crops_number=8, global_crops_size=224,
                 local_crops_size=96, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, max_side=1024, generator=None):
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("DinoAugment: `mean` and `std` take three values each")
        if int(local_crops_number) < 0:
            raise ValueError("DinoAugment: `local_crops_number` must not be negative")
        if int(max_side) < 1:
            raise ValueError("DinoAugment: `max_side` must be at least 1")
        for name, S in (("global_crops_size", global_crops_size), ("local_crops_size", local_crops_size)):
            if int(S) < 5:
                raise ValueError(f"DinoAugment: `{name}` must be at least 5 (the blur's reflect padding of 4), got {S}")
            if int(S) > 4096:
                raise ValueError(f"DinoAugment: `{name}` above 4096 is not supported, got {S}")
            if max_resize_taps(int(max_side), int(S)) > ops.dino_resize_max_taps(int(S)):
                raise ValueError(f"DinoAugment: `max_side` {max_side} needs {max_resize_taps(int(max_side), int(S))} taps at {name} "
                                 f"{S}; the resize kernel holds {ops.dino_resize_max_taps(int(S))}")
        self.global_crops_scale, self.local_crops_scale = tuple(global_crops_scale), tuple(local_crops_scale)
        self.local_crops_number = int(local_crops_number)
        self.global_crops_size, self.local_crops_size = int(global_crops_size), int(local_crops_size)
        self.mean = tuple(float(_f32(v)) for v in mean)
        self.std = tuple(float(_f32(v)) for v in std)
        self.max_side = int(max_side)
        self.generator = generator
        self._tables, self._workspaces, self._uploaded = {}, {}, {}

    # ---- the host side -------------------------------------------------------------------------------------------------
    def _check_sizes(self, heights, widths):
        heights = np.ascontiguousarray(heights, dtype=np.int64).reshape(-1)
        widths = np.ascontiguousarray(widths, dtype=np.int64).reshape(-1)
        if heights.shape != widths.shape or len(heights) == 0:
            raise ValueError("DinoAugment: heights and widths must be [B] each, B >= 1")
        if min(heights.min(), widths.min()) < 1:
            raise ValueError("DinoAugment: a source has a side below 1")
        if max(heights.max(), widths.max()) > self.max_side:
            raise ValueError(f"DinoAugment: a source side of {max(heights.max(), widths.max())} exceeds `max_side` = {self.max_side} "
                             "(the loader bounds the sources; raise max_side at construction)")
        return heights, widths

    def _draw_crop(self, p, c, b, H, W, scale, blur_p, may_solarize):
        g = self.generator
        p.box[c, b] = _crop_box(H, W, scale, g)
        p.flip[c, b] = bool(torch.rand(1, generator=g) < 0.5)
        if not 0.8 < torch.rand(1, generator=g):
            p.jitter[c, b] = True
            p.order[c, b] = torch.randperm(4, generator=g).numpy()
            p.brightness[c, b] = _uniform(0.6, 1.4, g)
            p.contrast[c, b] = _uniform(0.6, 1.4, g)
            p.saturation[c, b] = _uniform(0.8, 1.2, g)
            p.hue[c, b] = _uniform(-0.1, 0.1, g)
        p.gray[c, b] = bool(torch.rand(1, generator=g) < 0.2)
        if not (1 - blur_p) < torch.rand(1, generator=g):       # the reference's GaussianBlur(p): RandomApply(p = 1 - p)
            p.blur[c, b] = True
            p.sigma[c, b] = _uniform(0.1, 2.0, g)
        if may_solarize:
            p.solarize[c, b] = bool(torch.rand(1, generator=g) < 0.2)

    def draw(self, heights, widths):
        """One draw for B sources of the given sizes, image by image in the reference's order."""
        heights, widths = self._check_sizes(heights, widths)
        p = DinoAugParams(heights, widths, self.local_crops_number, self.global_crops_size, self.local_crops_size)
        for b in range(len(p)):
            H, W = int(heights[b]), int(widths[b])
            self._draw_crop(p, 0, b, H, W, self.global_crops_scale, 1.0, False)
            self._draw_crop(p, 1, b, H, W, self.global_crops_scale, 0.1, True)
            for c in range(2, 2 + self.local_crops_number):
                self._draw_crop(p, c, b, H, W, self.local_crops_scale, 0.5, False)
        return p

    # ---- the device side -----------------------------------------------------------------------------------------------
    def coef_capacity(self, B):
        """int32 words of the coefficient pool that B sources of up to ``max_side`` can need."""
        words = 0
        for S, n in ((self.global_crops_size, 2), (self.local_crops_size, self.local_crops_number)):
            words += n * B * 2 * (2 * S + S * max_resize_taps(self.max_side, S))
        return max(words, 1)

    def device_tables(self, B, device):
        """The device tables of a batch of B (fixed addresses: what a captured step reads) with their pinned staging."""
        key = (int(B), str(device))
        t = self._tables.get(key)
        if t is None:
            shapes = {"rows_global": (2 * B, ROW_WORDS), "rows_local": (max(self.local_crops_number * B, 1), ROW_WORDS),
                      "coef": (self.coef_capacity(B),)}
            t = self._tables[key] = {k: (torch.zeros(s, dtype=torch.int32, device=device), torch.zeros(s, dtype=torch.int32).pin_memory())
                                     for k, s in shapes.items()}
        return t

    def upload(self, tables, device):
        """Host tables (``DinoAugParams.tables()``) -> the device tables; only the used part of the pool travels."""
        B = tables["rows_global"].shape[0] // 2
        dev = self.device_tables(B, device)
        if tables["coef"].size > dev["coef"][0].numel():
            raise ValueError("DinoAugment: the coefficient pool exceeds the capacity `max_side` fixes")
        return upload_tables(dev, tables, self._uploaded, device)

    def _workspace(self, N, H, W, device, crops=True):
        """(workspace, uint8 crops buffer) of one launch, kept per shape AND stream: calls on different streams get buffers of
        their own, calls on one stream are ordered by it."""
        key = (N, H, W, str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._workspaces.get(key)
        if ws is None:
            ws = self._workspaces[key] = [ops.dino_color_workspace(N, H, W, device), None]
        if crops and ws[1] is None:
            ws[1] = torch.empty(N, H, W, 3, dtype=torch.uint8, device=device)
        return ws

    def _out(self, N, S, device, uint8_out):
        return (torch.empty(N, S, S, 3, dtype=torch.uint8, device=device) if uint8_out else
                torch.empty(N, 3, S, S, dtype=torch.float32, device=device))

    def launch(self, data, rows_global, rows_local, coef, out_global=None, out_local=None, uint8_out=False):
        """The launches alone, for device tables only (what a captured step records): ``data`` the packed uint8 images,
        ``rows_*`` int32 [N, ROW_WORDS], ``coef`` the pool."""
        for name, t in (("data", data), ("rows_global", rows_global), ("rows_local", rows_local), ("coef", coef)):
            if not torch.is_tensor(t):
                raise TypeError(f"DinoAugment.launch: `{name}` must be a device tensor, got {type(t).__name__}")
            _require_gpu(t, f"DinoAugment.launch: `{name}`")
        if data.dtype != torch.uint8:
            raise TypeError(f"DinoAugment.launch: `data` must be uint8, got {data.dtype}")
        outs = []
        for rows, S, out, n in ((rows_global, self.global_crops_size, out_global, 2), (rows_local, self.local_crops_size, out_local, self.local_crops_number)):
            if n == 0:
                outs.append(self._out(0, S, data.device, uint8_out))
                continue
            N = rows.shape[0]
            ws, crops = self._workspace(N, S, S, data.device)
            if out is None:
                out = self._out(N, S, data.device, uint8_out)
            ops.dino_resize_u8(data, rows, coef, S, crops)
            outs.append(ops.dino_color_u8(crops, rows, self.mean, self.std, out, ws))
        return tuple(outs)

    @staticmethod
    def _check_packed(packed, what):
        if not isinstance(packed, PackedImages):
            raise TypeError(f"{what}: `packed` must be a PackedImages (pack_images), got {type(packed).__name__}")
        _require_gpu(packed.data, f"{what}: `packed.data`")
        if packed.data.dtype != torch.uint8 or packed.data.dim() != 1:
            raise TypeError(f"{what}: `packed.data` must be a 1-D uint8 tensor, got {tuple(packed.data.shape)} {packed.data.dtype}")

    def apply(self, packed, params=None, uint8_out=False):
        """(global_crops [2 B, 3, G, G], local_crops [n B, 3, L, L]) normalised f32, crop-major as ``ssl.collate`` expects; with
        ``uint8_out`` the uint8 [*, S, S, 3] pixels in front of ToTensor.  params: a ``DinoAugParams`` (default: a fresh
        ``draw``).  The packed images are left untouched."""
        self._check_packed(packed, "DinoAugment.apply")
        heights, widths = self._check_sizes(*packed.host_sizes())
        if params is None:
            params = self.draw(heights, widths)
        elif not (np.array_equal(params.heights, heights) and np.array_equal(params.widths, widths)):
            raise ValueError("DinoAugment.apply: `params` were drawn for sources of other sizes")
        elif (params.n_local, params.global_size, params.local_size) != (self.local_crops_number, self.global_crops_size, self.local_crops_size):
            raise ValueError("DinoAugment.apply: `params` were drawn for another crop geometry")
        if int(heights @ widths) * 3 != packed.data.numel():
            raise ValueError("DinoAugment.apply: `packed.data` does not hold the images its sizes describe")
        t = self.upload(params.tables(), packed.data.device)
        return self.launch(packed.data, t["rows_global"], t["rows_local"], t["coef"], uint8_out=uint8_out)

    def apply_crops(self, crops_u8, params_rows, uint8_out=False):
        """The chain behind the resize (ColorJitter, grayscale, blur, solarize, output) on given uint8 [N, H, W, 3] crops, for
        tests and for callers who crop elsewhere.  params_rows: int32 [N, ROW_WORDS] (``DinoAugParams.color_rows``), numpy or
        device tensor.  The crops are left untouched."""
        if not torch.is_tensor(crops_u8) or crops_u8.dtype != torch.uint8 or crops_u8.dim() != 4 or crops_u8.shape[3] != 3:
            got = f"{tuple(crops_u8.shape)} {crops_u8.dtype}" if torch.is_tensor(crops_u8) else type(crops_u8).__name__
            raise TypeError(f"DinoAugment.apply_crops: `crops_u8` must be a uint8 [N, H, W, 3] tensor, got {got}")
        _require_gpu(crops_u8, "DinoAugment.apply_crops: `crops_u8`")
        N, H, W, _ = crops_u8.shape
        if min(H, W) < 5:
            raise ValueError(f"DinoAugment.apply_crops: crops below 5 pixels a side are refused (the blur's reflect padding), got {H} x {W}")
        rows = params_rows if torch.is_tensor(params_rows) else torch.from_numpy(np.ascontiguousarray(params_rows, dtype=np.int32))
        rows = rows.to(crops_u8.device)
        out = (torch.empty(N, H, W, 3, dtype=torch.uint8, device=crops_u8.device) if uint8_out else
               torch.empty(N, 3, H, W, dtype=torch.float32, device=crops_u8.device))
        return ops.dino_color_u8(crops_u8.contiguous(), rows, self.mean, self.std, out, self._workspace(N, H, W, crops_u8.device, crops=False)[0])

    def collate(self, packed, mask_ratio_tuple, mask_probability, n_tokens, mask_generator, params=None):
        """The dictionary of ``ssl.collate`` (what ``SSLTrainer.step`` takes) with the crops made on the device; the iBOT masks
        are ``ssl.collate``'s host code, moved to the crops' device."""
        gc, lc = self.apply(packed, params)
        out = _ssl.collate(gc, lc, mask_ratio_tuple, mask_probability, n_tokens, mask_generator)
        return {k: (v.to(gc.device) if torch.is_tensor(v) else v) for k, v in out.items()}

    def __call__(self, packed):
        return self.apply(packed)
