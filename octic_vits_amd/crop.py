"""The DeiT-III crops and the evaluation resize on the device, from a ragged batch of decoded uint8 images.

The reference crops on loader workers, one PIL bicubic resample per image: ``RandomResizedCropAndInterpolation(224, scale=(0.08, 1),
'bicubic')`` or, with ``--src``, ``Resize`` + ``RandomCrop(padding=4, reflect)`` in training (``deit/augment.py:97-108``),
``Resize(int(S / eval_crop_ratio), bicubic)`` + ``CenterCrop(S)`` in evaluation (``deit/datasets.py:119-125``;
``dinov2/data/transforms.py:77-91``), and behind that ``RandomRotate90`` / ``RandomHorizontalFlip(p=1)`` for ``--rot-eval`` /
``--flop-eval`` (``deit/datasets.py:91-96,127-132``).  Here the decoded sources go to the device as they are
(``dino_augment.pack_images``) and every one of these is ONE launch of csrc/crop.hip: a window of the reflect-padded, resized box of
a source, turned and mirrored, as uint8 [B, H, W, 3] (what ``augment.ThreeAugment`` takes) or as the normalised f32 [B, 3, H, W]
batch (what the model takes).  The kernel reproduces Pillow's 8-bit two-pass bicubic resample bit for bit (the contract is in
include/octic_hip.h; tests/golden/crop_numpy.py restates it, tests/golden/crop.npz holds PIL's pixels).

THE DRAW stays on the host and consumes the random streams as the reference does, image by image:

* ``RandomResizedCrop``: timm's ``RandomResizedCropAndInterpolation.get_params`` on PYTHON's ``random`` (torchvision's variant,
  ``dino_augment._crop_box``, draws from torch): up to 10 tries of ``random.uniform(*scale)`` (area) and
  ``exp(random.uniform(log r0, log r1))`` (aspect); a try with w <= W and h <= H draws ``random.randint(0, H - h)``, then
  ``random.randint(0, W - w)``; else the central-crop fallback.  timm is not a dependency: its published algorithm is the contract.
* ``SrcCrop``: ``RandomCrop.get_params`` on the padded resized size: nothing when both sides equal ``size``, else
  ``torch.randint(0, ph - size + 1)``, then ``torch.randint(0, pw - size + 1)``.
* ``EvalTransform``: with ``rot`` one ``random.choice([0, 90, 180, 270])`` per image; nothing else.

The host also computes the integer resampling coefficients (``dino_augment.resize_coeffs``: Pillow's ``precompute_coeffs`` in
float64, host code of the library).  Not built: decoding, the sampler (``RASampler``), antialiased or tensor-mode torchvision
resizing, timm's other interpolation modes.  There is no CPU path.
"""
import math
import random

import numpy as np
import torch

from . import ops
from .augment import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD
from .dino_augment import PackedImages, _require_gpu, resize_coeffs, resize_taps, upload_tables

__all__ = ["CropParams", "RandomResizedCrop", "SrcCrop", "EvalTransform", "make_classification_eval_transform", "resize_size",
           "center_crop_offset", "ROW_WORDS"]

ROW_WORDS = ops.CROP_ROW_WORDS
_f32 = np.float32
_POOL_MAX = (1 << 31) - 1


def resize_size(height, width, size):
    """torchvision's ``Resize(int)``: the shorter side becomes ``size``, the longer ``int(size * long / short)``: (rh, rw)."""
    height, width, size = int(height), int(width), int(size)
    short, long = (width, height) if width <= height else (height, width)
    new_long = int(size * long / short)
    return (new_long, size) if width <= height else (size, new_long)


def center_crop_offset(side, size):
    """torchvision's ``CenterCrop``: ``int(round((side - size) / 2.0))`` with Python's round (half to even)."""
    return int(round((int(side) - int(size)) / 2.0))


# ------------------------------------------------------------------------------------------------ one draw
class CropParams:
    """N output images of ``out_h`` x ``out_w`` from B sources, as numpy arrays: ``heights`` / ``widths`` int64 [B] (the
    sources), ``source`` int64 [N] (which source an output is cut from; default: output i from source i), ``box`` int32 [N, 4]
    (top, left, h, w: what is resampled), ``rsize`` int32 [N, 2] (rh, rw: to what size; default the output size), ``pad`` int32
    [N] (reflect padding round the resized box), ``win`` int32 [N, 2] (top, left of the output window in the padded resized box),
    ``rot`` int32 [N] (quarter turns counter-clockwise) and ``flip`` bool [N] (then mirrored along x)."""
    _FIELDS = (("box", np.int32, (4,)), ("rsize", np.int32, (2,)), ("pad", np.int32, ()), ("win", np.int32, (2,)), ("rot", np.int32, ()),
               ("flip", bool, ()))

    def __init__(self, heights, widths, out_h, out_w, box, source=None, **arrays):
        self.heights = np.ascontiguousarray(heights, dtype=np.int64).reshape(-1)
        self.widths = np.ascontiguousarray(widths, dtype=np.int64).reshape(-1)
        if self.heights.shape != self.widths.shape:
            raise ValueError("CropParams: heights and widths must be [B] each")
        self.out_h, self.out_w = int(out_h), int(out_w)
        self.box = np.ascontiguousarray(box, dtype=np.int32).reshape(-1, 4)
        N = self.box.shape[0]
        self.source = np.arange(N, dtype=np.int64) if source is None else np.ascontiguousarray(source, dtype=np.int64).reshape(-1)
        if self.source.shape != (N,) or N == 0 or self.source.min() < 0 or self.source.max() >= len(self.heights):
            raise ValueError("CropParams: `source` must name one of the B sources for each of the N >= 1 boxes")
        for name, dt, tail in self._FIELDS[1:]:
            if name in arrays:
                v = np.ascontiguousarray(arrays.pop(name), dtype=dt)
                if v.shape != (N,) + tail:
                    raise ValueError(f"CropParams: {name} must be {(N,) + tail}, got {v.shape}")
            else:
                v = np.zeros((N,) + tail, dt)
                if name == "rsize":
                    v[:] = (self.out_h, self.out_w)
            setattr(self, name, v)
        if arrays:
            raise TypeError(f"CropParams: unknown fields {sorted(arrays)}")

    def __len__(self):
        return int(self.box.shape[0])

    def __eq__(self, other):
        return (isinstance(other, CropParams) and (self.out_h, self.out_w) == (other.out_h, other.out_w) and
                np.array_equal(self.heights, other.heights) and np.array_equal(self.widths, other.widths) and
                np.array_equal(self.source, other.source) and all(np.array_equal(getattr(self, n), getattr(other, n)) for n, _, _ in self._FIELDS))

    def case(self, i):
        """Output i as the parameter dict of tests/golden/crop_numpy.py."""
        return dict(box=tuple(int(v) for v in self.box[i]), rsize=tuple(int(v) for v in self.rsize[i]), pad=int(self.pad[i]),
                    win=tuple(int(v) for v in self.win[i]), out=(self.out_h, self.out_w), rot=int(self.rot[i]), flip=bool(self.flip[i]))

    def tables(self):
        """What the kernel reads (``octic_crop_row`` and the coefficient pool, include/octic_hip.h), packed on the host: ``rows``
        int32 [N, ROW_WORDS] and ``coef`` int32 1-D (one block per distinct (length, resized length) of the batch).  Row words:
        src_offset (2) | src_h src_w | top left h w | rh rw | pad | win_top win_left | rot flip | hcoef htaps vcoef vtaps | 0."""
        N, OH, OW = len(self), self.out_h, self.out_w
        if min(OH, OW) < 5 or max(OH, OW) > 4096:
            raise ValueError(f"CropParams: output sizes are 5 .. 4096 a side, got {OH} x {OW}")
        max_taps = ops.crop_resize_max_taps(OW)
        offsets = np.concatenate([[0], np.cumsum(self.heights * self.widths * 3)[:-1]]).astype(np.int64)
        rows = np.zeros((N, ROW_WORDS), np.int32)
        pool, at, blocks = [], 0, {}
        for i in range(N):
            b = int(self.source[i])
            H, W = int(self.heights[b]), int(self.widths[b])
            top, left, h, w = (int(v) for v in self.box[i])
            rh, rw = (int(v) for v in self.rsize[i])
            pad, (wt, wl), rot = int(self.pad[i]), (int(v) for v in self.win[i]), int(self.rot[i])
            if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W):
                raise ValueError(f"CropParams: box {(top, left, h, w)} of output {i} leaves its {H} x {W} source")
            if rh < 1 or rw < 1:
                raise ValueError(f"CropParams: output {i} is resized to {rh} x {rw}")
            if pad < 0 or (pad > 0 and pad >= min(rh, rw)):
                raise ValueError(f"CropParams: reflect padding {pad} of output {i} must be below its resized sides {rh} x {rw}")
            if not (wt >= 0 and wl >= 0 and wt + OH <= rh + 2 * pad and wl + OW <= rw + 2 * pad):
                raise ValueError(f"CropParams: the {OH} x {OW} window at {(wt, wl)} of output {i} leaves its padded {rh + 2 * pad} x "
                                 f"{rw + 2 * pad} image")
            if not 0 <= rot <= 3 or (rot & 1 and OH != OW):
                raise ValueError(f"CropParams: rot must be 0 .. 3, and 1 or 3 need a square output, got {rot} at {OH} x {OW}")
            rows[i, 0:2] = np.array([offsets[b]], np.int64).view(np.int32)
            rows[i, 2:15] = (H, W, top, left, h, w, rh, rw, pad, wt, wl, rot, bool(self.flip[i]))
            for word, n, r in ((15, w, rw), (17, h, rh)):
                if word == 17 and resize_taps(n, r) > max_taps:    # (the vertical pass reads its taps' rows from LDS)
                    raise ValueError(f"CropParams: resampling {n} -> {r} rows (output {i}) needs {resize_taps(n, r)} taps; the kernel "
                                     f"holds {max_taps} for windows {OW} wide")
                if (n, r) not in blocks:
                    bounds, k = resize_coeffs(n, r)
                    if np.abs(k).max() >= 1 << 23:            # (the kernel multiplies on the 24-bit unit; Pillow's stay below 2^22 (1 + lobes))
                        raise ValueError(f"CropParams: a coefficient of {n} -> {r} exceeds 24 bits")
                    if at + bounds.size + k.size > _POOL_MAX:
                        raise ValueError(f"CropParams: the coefficient pool of this batch exceeds {_POOL_MAX} int32 words; use a smaller batch")
                    blocks[(n, r)] = (at, k.shape[1])
                    pool += [bounds.reshape(-1), k.reshape(-1)]
                    at += bounds.size + k.size
                rows[i, word], rows[i, word + 1] = blocks[(n, r)]
        return {"rows": rows, "coef": np.ascontiguousarray(np.concatenate(pool), dtype=np.int32)}


# ------------------------------------------------------------------------------------------------ the transforms
class _Crop:
    """What the three transforms share: the device tables, the upload and the launch.  A subclass draws one image at a time
    (``draw_one(H, W)`` -> the fields of one ``CropParams`` entry) in the reference's stream order."""

    def __init__(self, size, mean, std):
        if len(mean) != 3 or len(std) != 3:
            raise ValueError(f"{type(self).__name__}: `mean` and `std` take three values each")
        if not 5 <= int(size) <= 4096:
            raise ValueError(f"{type(self).__name__}: `size` must be 5 .. 4096, got {size}")
        self.size = int(size)
        self.mean = tuple(float(_f32(v)) for v in mean)
        self.std = tuple(float(_f32(v)) for v in std)
        self._tables, self._uploaded = {}, {}

    # ---- the host side -------------------------------------------------------------------------------------------------
    def draw(self, heights, widths):
        """One draw for B sources of the given sizes, image by image."""
        heights = np.ascontiguousarray(heights, dtype=np.int64).reshape(-1)
        widths = np.ascontiguousarray(widths, dtype=np.int64).reshape(-1)
        if heights.shape != widths.shape or len(heights) == 0:
            raise ValueError(f"{type(self).__name__}: heights and widths must be [B] each, B >= 1")
        if min(heights.min(), widths.min()) < 1:
            raise ValueError(f"{type(self).__name__}: a source has a side below 1")
        return self.params(heights, widths, [self.draw_one(int(h), int(w)) for h, w in zip(heights, widths)])

    def params(self, heights, widths, drawn):
        """The ``CropParams`` of the per-image results of ``draw_one``."""
        fields = {k: [d[k] for d in drawn] for k in drawn[0]}
        return CropParams(heights, widths, self.size, self.size, **fields)

    # ---- the device side -----------------------------------------------------------------------------------------------
    def device_tables(self, N, words, device):
        """The device tables of N outputs with their pinned staging; the pool grows (in powers of two) with what a batch needs."""
        key = (int(N), str(device))
        t = self._tables.get(key)
        if t is None or t["coef"][0].numel() < words:
            shapes = {"rows": (N, ROW_WORDS), "coef": (1 << max(int(words) - 1, 1).bit_length(),)}
            t = self._tables[key] = {k: (torch.zeros(s, dtype=torch.int32, device=device), torch.zeros(s, dtype=torch.int32).pin_memory())
                                     for k, s in shapes.items()}
        return t

    def upload(self, tables, device):
        """Host tables (``CropParams.tables()``) -> the device tables, as ``DinoAugment.upload``."""
        dev = self.device_tables(tables["rows"].shape[0], tables["coef"].size, device)
        return upload_tables(dev, tables, self._uploaded, device)

    def launch(self, data, rows, coef, out=None, uint8_out=False):
        """The launch alone, for device tables: ``data`` the packed uint8 images, ``rows`` int32 [N, ROW_WORDS], ``coef`` the pool."""
        for name, t in (("data", data), ("rows", rows), ("coef", coef)):
            if not torch.is_tensor(t):
                raise TypeError(f"{type(self).__name__}.launch: `{name}` must be a device tensor, got {type(t).__name__}")
            _require_gpu(t, f"{type(self).__name__}.launch: `{name}`")
        N, S = rows.shape[0], self.size
        if out is None:
            out = (torch.empty(N, S, S, 3, dtype=torch.uint8, device=data.device) if uint8_out else
                   torch.empty(N, 3, S, S, dtype=torch.float32, device=data.device))
        elif (out.dtype == torch.uint8) != bool(uint8_out):
            raise TypeError(f"{type(self).__name__}: `out` is uint8 with uint8_out=True, float32 otherwise")
        return ops.crop_resize_u8(data, rows, coef, self.mean, self.std, out)

    def apply(self, packed, params=None, out=None, uint8_out=False):
        """The crops of a ``PackedImages`` in one launch: normalised f32 [B, 3, S, S], or with ``uint8_out`` the uint8 [B, S, S, 3]
        pixels.  params: a ``CropParams`` (default: a fresh ``draw``); out: the output buffer.  The sources are left untouched."""
        what = f"{type(self).__name__}.apply"
        if not isinstance(packed, PackedImages):
            raise TypeError(f"{what}: `packed` must be a PackedImages (pack_images), got {type(packed).__name__}")
        _require_gpu(packed.data, f"{what}: `packed.data`")
        if packed.data.dtype != torch.uint8 or packed.data.dim() != 1:
            raise TypeError(f"{what}: `packed.data` must be a 1-D uint8 tensor, got {tuple(packed.data.shape)} {packed.data.dtype}")
        heights, widths = (np.asarray(v, np.int64) for v in packed.host_sizes())
        if params is None:
            params = self.draw(heights, widths)
        elif not (np.array_equal(params.heights, heights) and np.array_equal(params.widths, widths)):
            raise ValueError(f"{what}: `params` were drawn for sources of other sizes")
        elif (params.out_h, params.out_w) != (self.size, self.size):
            raise ValueError(f"{what}: `params` were drawn for another output size")
        if int(heights @ widths) * 3 != packed.data.numel():
            raise ValueError(f"{what}: `packed.data` does not hold the images its sizes describe")
        t = self.upload(params.tables(), packed.data.device)
        return self.launch(packed.data, t["rows"], t["coef"], out=out, uint8_out=uint8_out)

    def __call__(self, packed, **kw):
        return self.apply(packed, **kw)


class RandomResizedCrop(_Crop):
    """timm's ``RandomResizedCropAndInterpolation(size, scale, ratio, 'bicubic')`` (the crop of ``deit/augment.py:104-106``).  timm
    is not installed here: its published ``get_params`` is the contract - it draws from PYTHON's ``random`` (``rng``: the module
    or a ``random.Random``), where torchvision's ``RandomResizedCrop`` draws from torch."""

    def __init__(self, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), rng=None, mean=IMAGENET_DEFAULT_MEAN,
                 std=IMAGENET_DEFAULT_STD):
        super().__init__(size, mean, std)
        self.scale, self.ratio = tuple(scale), tuple(ratio)
        self.rng = random if rng is None else rng

    def get_params(self, height, width):
        """(top, left, h, w) of one source, consuming ``rng`` as timm does."""
        r, area = self.rng, height * width
        for _ in range(10):
            target_area = r.uniform(*self.scale) * area
            log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
            aspect_ratio = math.exp(r.uniform(*log_ratio))
            w = int(round(math.sqrt(target_area * aspect_ratio)))
            h = int(round(math.sqrt(target_area / aspect_ratio)))
            if w <= width and h <= height:
                i = r.randint(0, height - h)
                j = r.randint(0, width - w)
                if h < 1 or w < 1:
                    raise ValueError(f"RandomResizedCrop: an empty {h} x {w} box was drawn from a {height} x {width} source (the "
                                     "reference fails on it too); give it larger sources")
                return i, j, h, w
        in_ratio = width / height
        if in_ratio < min(self.ratio):
            w = width
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = height
            w = int(round(h * max(self.ratio)))
        else:
            w, h = width, height
        return (height - h) // 2, (width - w) // 2, h, w

    def draw_one(self, height, width):
        return dict(box=self.get_params(height, width))


class SrcCrop(_Crop):
    """The ``--src`` crop (``deit/augment.py:97-100``): ``Resize(size, bicubic)`` + ``RandomCrop(size, padding, 'reflect')``.
    ``generator``: torch's global CPU generator (default) or a ``torch.Generator``."""

    def __init__(self, size=224, padding=4, generator=None, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
        super().__init__(size, mean, std)
        if not 0 <= int(padding) < self.size:
            raise ValueError(f"SrcCrop: `padding` must be 0 .. size - 1 (reflect padding stays below the resized side), got {padding}")
        self.padding, self.generator = int(padding), generator

    def draw_one(self, height, width):
        S, p = self.size, self.padding
        rh, rw = resize_size(height, width, S)
        ph, pw = rh + 2 * p, rw + 2 * p
        if ph == S and pw == S:
            top = left = 0                                    # RandomCrop.get_params: nothing drawn
        else:
            top = int(torch.randint(0, ph - S + 1, size=(1,), generator=self.generator).item())
            left = int(torch.randint(0, pw - S + 1, size=(1,), generator=self.generator).item())
        return dict(box=(0, 0, height, width), rsize=(rh, rw), pad=p, win=(top, left))


class EvalTransform(_Crop):
    """The evaluation transform (``deit/datasets.py:119-132``): ``Resize(resize_size or int(size / crop_ratio), bicubic)`` +
    ``CenterCrop(size)``, with ``rot`` a ``RandomRotate90`` (one ``random.choice([0, 90, 180, 270])`` per image from ``rng``; the
    turn is counter-clockwise, Pillow's exact transpose) and with ``flip`` a ``RandomHorizontalFlip(p=1.0)`` behind it, then
    ``ToTensor`` + ``Normalize``.  ``EvalTransform(...)(packed)`` is the normalised f32 [B, 3, S, S] batch in one launch."""

    def __init__(self, size=224, crop_ratio=0.875, rot=False, flip=False, resize_size=None, mean=IMAGENET_DEFAULT_MEAN,
                 std=IMAGENET_DEFAULT_STD, rng=None):
        super().__init__(size, mean, std)
        self.resize_size = int(self.size / crop_ratio) if resize_size is None else int(resize_size)
        if self.resize_size < self.size:
            raise ValueError(f"EvalTransform: the resized shorter side {self.resize_size} is below `size` {self.size} (CenterCrop would "
                             "pad; the reference's crop_ratio <= 1 never does)")
        self.rot, self.flip = bool(rot), bool(flip)
        self.rng = random if rng is None else rng

    def draw_one(self, height, width):
        S = self.size
        rh, rw = resize_size(height, width, self.resize_size)
        rot = self.rng.choice([0, 90, 180, 270]) // 90 if self.rot else 0
        return dict(box=(0, 0, height, width), rsize=(rh, rw), win=(center_crop_offset(rh, S), center_crop_offset(rw, S)), rot=rot,
                    flip=self.flip)


def make_classification_eval_transform(resize_size=256, crop_size=224, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD):
    """``dinov2/data/transforms.py:77-91``: ``Resize(resize_size, bicubic)`` + ``CenterCrop(crop_size)`` + ``ToTensor`` + ``Normalize``."""
    return EvalTransform(size=crop_size, resize_size=resize_size, mean=mean, std=std)
