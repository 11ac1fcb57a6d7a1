"""LayerNormD8 kernel matrix: the case tables, the routing rule and the float64 references that
tests/test_layernorm_d8_host.py (CPU) and tests/test_layernorm_d8_matrix_gpu.py (GPU) share.

Everything here is plain data or numpy float64 arithmetic.  The references are written from the formulas
in the header comment of csrc/layernorm.hip and SURVEY.md section 10.3, NOT from autograd; the host test
holds them against the oracle (oracle/octic_ref.py LayerNormD8 in float64 + autograd).

A row is the packed layout of include/octic_hip.h: [A1 | A2 | B1 | B2 | E_row0 | E_row1], 8c columns;
alpha5 = (A1, A2, B1, B2: [c]; E: [2c], shared by both E rows); beta: [c], added to A1 only.
"""
import zlib

import numpy as np
import torch

import cases

# ------------------------------------------------------------------------------------------- tables
# lane-group ("g8") kernels: packed rows, c % 32 == 0, NV = c / 32 chunks per lane
G8_C = [32, 64, 96, 128, 160, 192, 224, 256]
# generic kernels: NV = 2 (c <= 64), 4 (c <= 128), 5 (c <= 160), 8 (c <= 256).  72 and 168 are the first c of NV = 4 and 8:
# lanes 16..63 (resp. 32..63) own a last chunk beyond the row.  56, 120, 152, 248 are the last c of each NV.
GENERIC_C = [8, 56, 72, 120, 136, 152, 168, 200, 248]
# c % 32 == 0 shapes that only a non-packed view sends down the generic kernel
TUPLE_G8_C = [32, 160]
# octic_layernorm_d8_bwd_cast serves the wide kernel only
CAST_C = [32, 64, 96, 128, 160]
CAST_REFUSED = [("packed", 192), ("packed", 48), ("tuple", 32)]

# one wave per row; the backward block has 8 waves, the forward block 4: idle waves (M < 8), one full block, one row past it,
# and a second round of blocks
SMALL_M = [1, 7, 8, 9, 33]
# the backward grid is capped at 256 blocks x 8 waves, the forward grid at 4096 x 4: the last M without a second trip of the
# row loop, the first with one, and (backward) one with a third trip for a few waves only
BWD_STRIDE_M = [2048, 2049, 4100]
FWD_STRIDE_M = [16384, 16385]
BWD_WAVES, BWD_CAP = 8, 256

LAYOUTS = ["packed", "packed_ld", "tuple", "tuple_ld", "mixed"]
AFFINE = ["alpha_beta", "alpha", "none"]
KINDS = ["normal", "offset1000", "const_row"]

# ln_bwd_finish_body: 16 block-lanes; four slabs in flight while b + 48 < nblk, then a tail of one slab per trip
FINISH_NBLK = [1, 2, 15, 16, 17, 47, 48, 49, 63, 64, 65, 113, 256]
FINISH_C = [8, 24, 160]         # 7c is a multiple of the 16 outputs of a block only at c = 160
BATCH_JOBS, BATCH_C = 50, [8, 160, 24, 96]

EPS = 1e-5
SQRT2_OVER_4 = np.sqrt(2.0) / 4.0


def bwd_blocks(M):
    return max(1, min(BWD_CAP, (M + BWD_WAVES - 1) // BWD_WAVES))


# ------------------------------------------------------------------------------------------ routing
def pick_nv(c):
    need = (2 * c + 63) // 64           # 16-byte chunks of a row per lane
    for nv in (2, 4, 5, 8):
        if need <= nv:
            return nv
    return 0


def route(c, packed, g_dtype=None, cast=False, mask=False):
    """(kernel, NV) of a launch: forward with g_dtype None, backward with g_dtype "f32" | "bf16".
    packed: every view of the call is one packed tensor (any row stride).  cast: octic_layernorm_d8_bwd_cast.
    mask: a sample mask is given.  ("refused", 0) where the entry point returns OCTIC_ESHAPE."""
    if c <= 0 or c % 8 or pick_nv(c) == 0:
        return ("refused", 0)
    g8 = packed and c % 32 == 0 and c <= 256
    if g_dtype is None:
        if g8:
            return ("ln_fwd_g8", c // 32)
        return ("ln_fwd_pk" if packed else "ln_fwd_tuple", pick_nv(c))
    if cast and g_dtype != "bf16":
        return ("refused", 0)
    if g8:
        if g_dtype == "bf16" and c // 32 <= 5:
            return ("ln_bwd_g8_wide_mask" if mask else "ln_bwd_g8_wide", c // 32)
        if cast:
            return ("refused", 0)
        return ("ln_bwd_g8_f32" if g_dtype == "f32" else "ln_bwd_g8_bf16_narrow", c // 32)
    if cast:
        return ("refused", 0)
    return (("ln_bwd_pk_" if packed else "ln_bwd_tuple_") + g_dtype, pick_nv(c))      # the mask is a permission: all rows read


def layout_is_packed(layout):
    return layout in ("packed", "packed_ld")


def matrix_c(layout):
    """The channel counts the GPU matrix runs in a layout."""
    return G8_C + GENERIC_C if layout_is_packed(layout) else GENERIC_C + TUPLE_G8_C


# every instance the tables must reach: {kernel: set of NV}
REQUIRED = {
    "ln_fwd_g8": set(range(1, 9)),
    "ln_bwd_g8_f32": set(range(1, 9)),
    "ln_bwd_g8_bf16_narrow": {6, 7, 8},
    "ln_bwd_g8_wide": {1, 2, 3, 4, 5},
    "ln_bwd_g8_wide_mask": {1, 2, 3, 4, 5},
    "ln_fwd_pk": {2, 4, 5, 8},
    "ln_fwd_tuple": {2, 4, 5, 8},
    "ln_bwd_pk_f32": {2, 4, 5, 8},
    "ln_bwd_pk_bf16": {2, 4, 5, 8},
    "ln_bwd_tuple_f32": {2, 4, 5, 8},
    "ln_bwd_tuple_bf16": {2, 4, 5, 8},
}
MASK_C = [32, 64, 96, 128, 160]      # tests/test_row_skip_gpu.py test_octic_layernorm_bwd_equals_the_unmasked_launch


def reached():
    """{kernel: set of NV} over everything the GPU matrix launches, counted through route()."""
    got = {}

    def add(r):
        got.setdefault(r[0], set()).add(r[1])

    for layout in LAYOUTS:
        pk = layout_is_packed(layout)
        for c in matrix_c(layout):
            add(route(c, pk))
            for gd in ("f32", "bf16"):
                add(route(c, pk, gd))
    for c in CAST_C:
        add(route(c, True, "bf16", cast=True))
    for c in MASK_C:
        add(route(c, True, "bf16", mask=True))
    return got


# ---------------------------------------------------------------------------------------- references
def segments(c):
    """(first column, last column + 1, n, w) of the six segments of a packed row."""
    return [(0, c, c, 1.0), (c, 2 * c, c, 1.0), (2 * c, 3 * c, c, 1.0), (3 * c, 4 * c, c, 1.0),
            (4 * c, 6 * c, 2 * c, 0.5), (6 * c, 8 * c, 2 * c, 0.5)]


def alpha_row(alpha5, c):
    """alpha by packed column ([8c] float64), ones without affine."""
    if alpha5 is None:
        return np.ones(8 * c)
    a = [np.asarray(t, np.float64) for t in alpha5]
    return np.concatenate([a[0], a[1], a[2], a[3], a[4], a[4]])


def _moments(x, eps):
    M, D = x.shape
    c = D // 8
    mean = np.empty((M, 6))
    xc = np.empty_like(x)
    S = np.full(M, float(eps))
    for k, (lo, hi, n, w) in enumerate(segments(c)):
        mean[:, k] = x[:, lo:hi].sum(1) / n
        xc[:, lo:hi] = x[:, lo:hi] - mean[:, k:k + 1]
        S += w * (xc[:, lo:hi] ** 2).sum(1) / n
    return mean, xc, S


def ln_ref(x, alpha5, beta, eps=EPS):
    """x [M, 8c] -> (y [M, 8c], mean [M, 6], rstd [M]) in float64."""
    x = np.asarray(x, np.float64)
    c = x.shape[1] // 8
    mean, xc, S = _moments(x, eps)
    rstd = 1.0 / (SQRT2_OVER_4 * np.sqrt(S))
    y = xc * rstd[:, None] * alpha_row(alpha5, c)
    if beta is not None:
        y[:, :c] += np.asarray(beta, np.float64)
    return y, mean, rstd


def ln_bwd_ref(g, x, alpha5, dres, eps=EPS):
    """(dx [M, 8c], dalpha5, dbeta [c]) in float64; dx = dres + LN'(g)."""
    g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
    c = x.shape[1] // 8
    mean, xc, S = _moments(x, eps)
    rstd = 1.0 / (SQRT2_OVER_4 * np.sqrt(S))
    xh = xc * rstd[:, None]
    gh = g * alpha_row(alpha5, c)
    dstd = -(gh * xh).sum(1) * rstd
    dS = dstd * rstd / 16.0
    dx = np.empty_like(x)
    for lo, hi, n, w in segments(c):
        ghs = gh[:, lo:hi]
        dx[:, lo:hi] = (ghs - ghs.sum(1, keepdims=True) / n) * rstd[:, None] + (w * 2.0 / n) * dS[:, None] * xc[:, lo:hi]
    if dres is not None:
        dx += np.asarray(dres, np.float64)
    P = (g * xh).sum(0)
    dalpha5 = [P[i * c:(i + 1) * c] for i in range(4)] + [P[4 * c:6 * c] + P[6 * c:8 * c]]
    return dx, dalpha5, g[:, :c].sum(0)


def param_term_sums(g, x, eps=EPS):
    """sum over rows of |term| for every parameter-gradient column: (five arrays like dalpha5, one like dbeta) - the scale an
    f32 sum of those terms is measured against."""
    g, x = np.asarray(g, np.float64), np.asarray(x, np.float64)
    c = x.shape[1] // 8
    _, xc, S = _moments(x, eps)
    T = np.abs(g * xc / (SQRT2_OVER_4 * np.sqrt(S))[:, None]).sum(0)
    return [T[i * c:(i + 1) * c] for i in range(4)] + [T[4 * c:6 * c] + T[6 * c:8 * c]], np.abs(g[:, :c]).sum(0)


# -------------------------------------------------------------------------------------------- inputs
def pack5(xs):
    """reference 5-tuple (leading dims [1, M]) -> packed [M, 8c]"""
    return torch.cat([xs[0], xs[1], xs[2], xs[3], xs[4].flatten(-2)], dim=-1)[0].contiguous()


def unpack5(t, c):
    return (t[..., :c], t[..., c:2 * c], t[..., 2 * c:3 * c], t[..., 3 * c:4 * c], t[..., 4 * c:].unflatten(-1, (2, 2 * c)))


def make_x(M, c, kind="normal"):
    """packed f32 [M, 8c]: seeded normals with a per-row, per-segment offset (cases.tuple5).  offset1000: mean >> spread.
    const_row: the middle row is constant, so its S is eps alone.  The constant is 0: with any other value the outcome would
    hang on whether n * fl(1/n) rounds to 1 in the kernel and on nothing the row is there for (mean removal is exercised by
    every other row, and at its worst by offset1000)."""
    x = pack5(cases.tuple5(f"ln_d8.x.{M}.{c}", 1, M, c))
    if kind == "offset1000":
        x = x + 1000.0
    elif kind == "const_row":
        x[M // 2] = 0.0
    elif kind != "normal":
        raise ValueError(kind)
    return x


def make_g(M, c, tag="g"):
    return pack5(cases.tuple5(f"ln_d8.{tag}.{M}.{c}", 1, M, c, False))


def make_int_g(M, c):
    """integers in [-8, 8]: exact in bf16 and f32, and so is every column sum of up to 2^20 rows"""
    gen = torch.Generator().manual_seed(zlib.crc32(f"ln_d8.ig.{M}.{c}".encode()) & 0x7FFFFFFF)
    return torch.randint(-8, 9, (M, 8 * c), generator=gen).float()


def make_affine(c):
    """alpha5, beta (f32) with a distinct value in every column: alpha walks 0.5 .. 1.5 over the 6c parameters in
    order A1, A2, B1, B2, E; beta walks 0.25 .. 1.25."""
    a = 0.5 + torch.arange(6 * c, dtype=torch.float64) / (6 * c)
    alpha5 = [a[i * c:(i + 1) * c].float().contiguous() for i in range(4)] + [a[4 * c:].float().contiguous()]
    beta = (0.25 + torch.arange(c, dtype=torch.float64) / c).float().contiguous()
    return alpha5, beta
