"""The arithmetic contract of csrc/augment.hip restated with numpy integers and float32: what the kernels must compute, bit for
bit, and what PIL computes (tests/test_augment_host.py holds it against the golden file and against live PIL).  No PIL here:
the GPU tests import this module on a machine without the reference."""
import numpy as np

f32 = np.float32


def luma(px):
    """PIL's convert("L") of uint8 [..., 3]: (19595 R + 38470 G + 7471 B + 0x8000) >> 16, as int64."""
    p = px.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16


def blur_constants(radius):
    """(r, ww, fw) of one box pass of ImageFilter.GaussianBlur(radius): float32 at every operation."""
    rho = f32(radius)
    s2 = f32(f32(rho * rho) / f32(3))
    L = f32(np.sqrt(f32(f32(f32(12) * s2) + f32(1))))
    l = f32(np.floor(f32(f32(L - f32(1)) / f32(2))))
    a = f32(f32(f32(f32(2) * l) + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * s2)))
    lp = f32(l + f32(1))
    a = f32(a / f32(f32(6) * f32(s2 - f32(lp * lp))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(f32(f32(1 << 24) / f32(f32(fr * f32(2)) + f32(1))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def box_pass(a, r, ww, fw):
    """One extended-box pass along the LAST axis of an integer array holding uint8 values."""
    n = a.shape[-1]
    x = np.arange(n)
    acc = np.zeros(a.shape, dtype=np.int64)
    for d in range(-r, r + 1):
        acc += a[..., np.clip(x + d, 0, n - 1)]
    edge = a[..., np.clip(x - r - 1, 0, n - 1)] + a[..., np.clip(x + r + 1, 0, n - 1)]
    return (ww * acc + fw * edge + (1 << 23)) >> 24


def blur(px, r, ww, fw):
    """uint8 [H, W, 3] -> three passes along x, then three along y, per channel; uint8 between the passes."""
    a = px.astype(np.int64).transpose(2, 0, 1)              # [3, H, W]
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    a = a.transpose(0, 2, 1)
    for _ in range(3):
        a = box_pass(a, r, ww, fw)
    return a.transpose(2, 1, 0).astype(np.uint8)            # [3, W, H] -> [H, W, 3]


def blend(deg, px, factor):
    """Image.blend(degenerate, image, factor): deg + f (v - deg) in f32 with separately rounded product and sum, clipped to
    [0, 255], truncated."""
    deg = np.asarray(deg).astype(f32)
    t = (deg + (f32(factor) * (px.astype(f32) - deg)).astype(f32)).astype(f32)
    return np.clip(t, f32(0), f32(255)).astype(np.uint8)


def apply_u8(px, params):
    """uint8 [H, W, 3] and one parameter dict (tests/golden/augment_case.py) -> the augmented uint8 [H, W, 3]."""
    px = np.ascontiguousarray(px, dtype=np.uint8)
    H, W, _ = px.shape
    if params["flip"]:
        px = px[:, ::-1]
    op = int(params["op"])
    if op == 1:
        px = np.repeat(luma(px)[..., None], 3, axis=-1).astype(np.uint8)
    elif op == 2:
        px = np.where(px < 128, px, 255 - px).astype(np.uint8)
    elif op == 3:
        px = blur(px, *blur_constants(params["radius"]))
    for fn in params["order"]:
        if fn == 0:
            px = blend(0, px, params["brightness"])
        elif fn == 1:
            S, N = int(luma(px).sum()), H * W
            px = blend((2 * S + N) // (2 * N), px, params["contrast"])
        elif fn == 2:
            px = blend(luma(px)[..., None], px, params["saturation"])
    return np.ascontiguousarray(px)


def normalize(u8, mean, std):
    """ToTensor + Normalize: uint8 [..., H, W, 3] -> f32 [..., 3, H, W] = (v / 255 - mean) / std, two f32 divisions."""
    v = u8.astype(f32) / f32(255)
    out = (v - np.asarray(mean, dtype=f32)) / np.asarray(std, dtype=f32)
    return np.ascontiguousarray(np.moveaxis(out.astype(f32), -1, -3))
