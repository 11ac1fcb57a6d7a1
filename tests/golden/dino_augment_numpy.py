"""The arithmetic contract of csrc/dino_augment.hip restated with numpy integers, float32 and float64: what the kernels must
compute and what Pillow / torchvision compute for the DINOv2 multi-crop augmentation (tests/golden/make_dino_augment_golden.py
holds it against live PIL; tests/test_dino_augment_host.py against the golden file).  No Pillow here: the GPU tests import this
module on a machine without it.

One crop's parameters (``params``, the dict of tests/golden/dino_augment_case.py): ``box`` (top, left, h, w), ``size`` S,
``flip``, ``jitter`` (bool), ``order`` (ColorJitter's ops in application order: 0 brightness, 1 contrast, 2 saturation, 3 hue),
``brightness``, ``contrast``, ``saturation``, ``hue``, ``gray``, ``blur`` (bool), ``sigma``, ``solarize``."""
import numpy as np

from augment_numpy import blend, luma, normalize  # noqa: F401  (the ImageEnhance arithmetic and the output are shared)

f32, f64 = np.float32, np.float64
PRECISION_BITS = 22
BLUR_BAND = 2.0 ** -9


# ------------------------------------------------------------------------------------------------ Pillow's 8-bit bicubic resample
def bicubic(t):
    a = -0.5
    t = abs(float(t))
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def resize_coeffs(n, S):
    """One axis, crop length n -> S: (xmin int32 [S], count int32 [S], k int32 [S, ksize]); float64 throughout."""
    scale = n / S
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = int(np.ceil(support)) * 2 + 1
    xmin, cnt, kk = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, ksize), np.int32)
    for x in range(S):
        center = (x + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n)
        w = [bicubic((j + lo - center + 0.5) / fs) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[x], cnt[x] = lo, hi - lo
        kk[x, :hi - lo] = [int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5) for v in w]
    return xmin, cnt, kk


def resample_last_axis(a, S):
    """uint8 [..., n] -> uint8 [..., S] along the last axis; n == S: the pass is skipped."""
    n = a.shape[-1]
    if n == S:
        return a
    xmin, cnt, kk = resize_coeffs(n, S)
    a = a.astype(np.int64)
    out = np.zeros(a.shape[:-1] + (S,), np.int64)
    for x in range(S):
        acc = (a[..., xmin[x]:xmin[x] + cnt[x]] * kk[x, :cnt[x]].astype(np.int64)).sum(-1)
        out[..., x] = np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)
    return out.astype(np.uint8)


def resized_crop(src, box, S):
    """img.crop(box).resize((S, S), BICUBIC): uint8 [H, W, 3] -> [S, S, 3]; horizontal pass, uint8, vertical pass."""
    top, left, h, w = (int(v) for v in box)
    c = np.ascontiguousarray(src[top:top + h, left:left + w]).transpose(0, 2, 1)    # [h, 3, w]
    c = resample_last_axis(c, S).transpose(2, 1, 0)                                 # [S, 3, h]
    return np.ascontiguousarray(resample_last_axis(c, S).transpose(2, 0, 1))        # [S(y), S(x), 3]


# ------------------------------------------------------------------------------------------------ Pillow's RGB <-> HSV
def _clip8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


def _round_half_away(x):
    """C round() of non-negative doubles."""
    fl = np.floor(x)
    return np.where(x - fl >= 0.5, fl + 1.0, fl)


def rgb_to_hsv(px):
    px = np.asarray(px, dtype=np.uint8)
    r, g, b = (px[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(f32)
        s = cr / maxc.astype(f32)
        rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
        h_r = bc - gc                                                               # float - float
        h_g = (2.0 + rc.astype(f64) - bc.astype(f64)).astype(f32)                   # double, stored to float
        h_b = (4.0 + gc.astype(f64) - rc.astype(f64)).astype(f32)
        h = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
        h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.where(grey, 0, np.clip(np.nan_to_num(h.astype(f64) * 255.0).astype(np.int64), 0, 255))
        S = np.where(grey, 0, np.clip(np.nan_to_num(s.astype(f64) * 255.0).astype(np.int64), 0, 255))
    return np.stack([H, S, maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    hsv = np.asarray(hsv, dtype=np.uint8)
    H, S, V = (hsv[..., i] for i in range(3))
    hf = H.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hf)
    f = (hf - i).astype(f32)
    fs = (S.astype(f32).astype(f64) / 255.0).astype(f32)
    v = V.astype(f64)
    fd, fsd = f.astype(f64), fs.astype(f64)
    p = _clip8(_round_half_away(v * (1.0 - fsd)))
    q = _clip8(_round_half_away(v * (1.0 - fsd * fd)))
    t = _clip8(_round_half_away(v * (1.0 - fsd * (1.0 - fd))))
    sel = i.astype(np.int64) % 6
    R = np.choose(sel, [V, q, p, p, t, V])
    G = np.choose(sel, [t, V, V, q, p, p])
    B = np.choose(sel, [p, p, t, V, V, q])
    grey = S == 0
    return np.stack([np.where(grey, V, R), np.where(grey, V, G), np.where(grey, V, B)], -1).astype(np.uint8)


def hue_shift(hue_factor):
    """torchvision's uint8 addend: (uint8)(int)(hue_factor 255), truncation toward zero, wrap mod 256."""
    return int(float(hue_factor) * 255) % 256


def adjust_hue(px, hue_factor):
    hsv = rgb_to_hsv(px)
    hsv[..., 0] = (hsv[..., 0].astype(np.int64) + hue_shift(hue_factor)) % 256
    return hsv_to_rgb(hsv)


# ------------------------------------------------------------------------------------------------ torchvision's GaussianBlur(9)
def blur_weights(sigma):
    """The nine f32 weights of torchvision's _get_gaussian_kernel1d(9, sigma), computed with torch as it does."""
    import torch
    x = torch.linspace(-4.0, 4.0, steps=9, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / float(sigma)).pow(2))
    return (pdf / pdf.sum()).numpy().astype(f32)


def blur_f64(px, weights):
    """uint8 [H, W, 3] -> float64 [H, W, 3]: the 81 products w_y w_x p of the f32 weights over the reflect-padded image."""
    H, W, _ = px.shape
    k = np.asarray(weights, dtype=f32).astype(f64)
    p = np.pad(px.astype(f64), ((4, 4), (4, 4), (0, 0)), mode="reflect")
    e = np.zeros((H, W, 3), f64)
    for dy in range(9):
        for dx in range(9):
            e += (k[dy] * k[dx]) * p[dy:dy + H, dx:dx + W]
    return e


def blur_candidates(px, weights):
    """(want, alt): rint(e), and the other neighbour wherever |frac(e) - 0.5| < 2^-9 (equal to want elsewhere)."""
    e = blur_f64(px, weights)
    want = np.rint(e)
    frac = e - np.floor(e)
    band = np.abs(frac - 0.5) < BLUR_BAND
    other = np.where(want > e, want - 1, want + 1)
    alt = np.where(band, other, want)
    return np.clip(want, 0, 255).astype(np.uint8), np.clip(alt, 0, 255).astype(np.uint8)


def solarize(px):
    return np.where(px < 128, px, 255 - px).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the chain
def color_chain(px, params):
    """The chain behind the resize on a uint8 [S, S', 3] crop -> (want, alt) uint8; alt differs from want only where a
    blurred pixel may round either way."""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    Hh, Ww, _ = px.shape
    if params["jitter"]:
        for fn in params["order"]:
            if fn == 0:
                px = blend(0, px, params["brightness"])
            elif fn == 1:
                S, N = int(luma(px).sum()), Hh * Ww
                px = blend((2 * S + N) // (2 * N), px, params["contrast"])
            elif fn == 2:
                px = blend(luma(px)[..., None], px, params["saturation"])
            elif fn == 3:
                px = adjust_hue(px, params["hue"])
    if params["gray"]:
        px = np.repeat(luma(px)[..., None], 3, axis=-1).astype(np.uint8)
    if params["blur"]:
        want, alt = blur_candidates(px, blur_weights(params["sigma"]))
    else:
        want = alt = px
    if params["solarize"]:
        want, alt = solarize(want), solarize(alt)
    return np.ascontiguousarray(want), np.ascontiguousarray(alt)


def apply_u8(src, params):
    """uint8 source [H, W, 3] and one crop's parameters -> (want, alt) uint8 [S, S, 3]."""
    c = resized_crop(np.asarray(src, dtype=np.uint8), params["box"], int(params["size"]))
    if params["flip"]:
        c = c[:, ::-1]
    return color_chain(c, params)
