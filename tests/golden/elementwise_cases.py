"""Elementwise / permutation kernel matrix (csrc/elementwise.hip): the case tables, the launch-routing formulas, the seeded
inputs and the float64 references that tests/test_elementwise_matrix_gpu.py runs (and tests/test_elementwise_cases_host.py
holds against each other on the CPU).

Everything here is plain data, torch on the CPU or the oracle (oracle/octic_ref.py) in float64.  A row is the packed layout
of include/octic_hip.h: [A1 | A2 | B1 | B2 | E_row0 | E_row1], 8c columns; the eight isotypic components of hidden channel j
are the columns j + k*c, k = 0..7 (comp_ptrs of elementwise.hip), so a packed row reshaped [8, c] has one group per column.
"""
import functools
import zlib

import numpy as np
import torch

import cases
from ln_d8_cases import pack5, unpack5
from oracle import octic_ref as R

LAYOUTS = ["packed", "packed_ld", "tuple", "tuple_ld"]
DTYPES = ["f32", "bf16"]
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
ESIZE = {"f32": 4, "bf16": 2}
GRID_CAP = 4096                      # grid_for: 256 CUs x 16 blocks of 256 threads, grid-stride beyond


def gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()) & 0x7FFFFFFF)


def grid_for(total):
    return max(1, min(GRID_CAP, (total + 255) // 256))


def second_item(total):
    """True where some thread of a grid_for(total) launch takes a second grid-stride item."""
    return total > GRID_CAP * 256


# ---------------------------------------------------------------------------------------------- 1. weight preparation
PREP_SHAPES = [(8, 8), (8, 24), (64, 64), (40, 120), (72, 32), (160, 640)]
PREP_TABLE3 = [(8, 24), (40, 120), (72, 32)]      # three shapes in one table; item i lacks cs / wb / wt (i = 0, 1, 2)
PREP_MANY = 300                                   # items of (8, 8): 1500 workgroups, two passes of the 256-wide item search
PREP_ITEM_DTYPE = np.dtype([("w", "<u8", 5), ("cs", "<u8", 5), ("wb", "<u8"), ("wt", "<u8"), ("cin", "<i4"), ("cout", "<i4"),
                            ("block_begin", "<i4"), ("block_count", "<i4")])      # octic_prep_item of include/octic_hip.h


def prep_tiles(cin, cout):
    t = lambda n: (n + 63) // 64
    return 4 * t(cout) * t(cin) + t(2 * cout) * t(2 * cin)


def prep_shapes5(cin, cout):
    """(N, K) of the five master matrices W_g [N, K]."""
    return [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]


def prep_inputs(tag, cin, cout):
    """(w5, cs5) f32: seeded normals; the layer scales are neither powers of two nor of one sign."""
    w5 = [torch.randn(n, k, generator=gen(f"ew.prep.w.{tag}.{cin}.{cout}.{g}")) for g, (n, k) in enumerate(prep_shapes5(cin, cout))]
    cs5 = [0.7 * torch.randn(n, generator=gen(f"ew.prep.cs.{tag}.{cin}.{cout}.{g}")) + 0.3
           for g, (n, _) in enumerate(prep_shapes5(cin, cout))]
    return w5, cs5


def prep_ref(w5, cs5, dtype):
    """(wb, wt) flat [8 cin cout] of the compute dtype: one f32 multiply and one rounding per element."""
    wb = torch.cat([w.to(dtype).flatten() for w in w5])
    wt = torch.cat([((w * cs[:, None]) if cs is not None else w).t().contiguous().to(dtype).flatten()
                    for w, cs in zip(w5, cs5 if cs5 is not None else [None] * 5)])
    return wb, wt


# ------------------------------------------------------------------------------------------------ 2. head pack / unpack
HEADS_SLOTS = (1, 2, 4, 5, 8, 16)
HEADS_T = [1, 3, 4, 5, 7]            # short last tiles of 1, 3, 1, 3 tokens, T < TT and T = TT (257 only at ViT-H below)
HEADS_MAX_LDS = 160 * 1024


def heads_route(dtype, c, H, n_s, direction):
    """heads_dispatch / heads_launch of elementwise.hip: (V, SLOTS, TT, LDS bytes), or ("refused", why) for OCTIC_ESHAPE.
    direction 0: pack (view -> heads), 1: unpack."""
    es = ESIZE[dtype]
    w = c // H
    V = 1
    while V * 2 <= 16 // es and w % (V * 2) == 0:
        V *= 2
    row_bytes = n_s * 8 * c * es
    TT = 4
    while TT > 1 and TT * row_bytes > 64 * 1024:
        TT >>= 1
    if TT * row_bytes > HEADS_MAX_LDS:
        return ("refused", "lds")
    se = 16 // es if direction == 1 else V
    slots = (TT * 8 * w // se + 63) // 64
    for sl in HEADS_SLOTS:
        if slots <= sl:
            return (V, sl, TT, TT * row_bytes)
    return ("refused", "slots")


def _divisors(n):
    small = [d for d in range(1, int(n ** 0.5) + 1) if n % d == 0]
    return sorted(set(small + [n // d for d in small]))


@functools.lru_cache(maxsize=None)
def heads_reachable():
    """{(dtype, V, direction, SLOTS): (c, H, n_s)} over every shape heads_check accepts whose token row fits the LDS: the
    first shape found walking c upwards, so the smallest c that selects the instantiation."""
    out = {}
    for dtype in DTYPES:
        cmax = HEADS_MAX_LDS // (8 * ESIZE[dtype])
        for c in range(8, cmax + 1, 8):
            for H in _divisors(c):
                for n_s in (1, 3):
                    for d in (0, 1):
                        r = heads_route(dtype, c, H, n_s, d)
                        if r[0] != "refused":
                            out.setdefault((dtype, r[0], d, r[1]), (c, H, n_s))
    return out


def heads_all_instances():
    return [(dt, V, d, sl) for dt in DTYPES for V in ((1, 2, 4) if dt == "f32" else (1, 2, 4, 8)) for d in (0, 1) for sl in HEADS_SLOTS]


def heads_cases():
    """[(dtype, B, T, H, c, n_s, layout)]; a case runs pack and then unpack.  Three parts: (a) the head widths w = 5, 10, 12, 8
    and 16 at every T, both n_s, layouts in turn; (b) the shapes named for SLOTS 5 / 8 / 16 and TT 2 / 1, all four layouts;
    (c) for every instantiation the launchers can select (heads_reachable) that (a) and (b) leave out, its smallest shape."""
    out = []
    k = 0
    for c, H in ((40, 8), (160, 16), (96, 8), (64, 8), (128, 8)):
        for dtype in DTYPES:
            for n_s in (1, 3):
                for T in HEADS_T:
                    out.append((dtype, 2, T, H, c, n_s, LAYOUTS[k % 4]))
                    k += 1
    for layout in LAYOUTS:
        for dtype in DTYPES:
            out.append((dtype, 2, 5, 8, 72, 3, layout))          # w = 9
            out.append((dtype, 2, 7, 8, 120, 1, layout))         # w = 15
            out.append((dtype, 1, 5, 8, 136, 3, layout))         # w = 17
            out.append((dtype, 2, 5, 8, 72, 1, layout))
        out.append(("f32", 2, 3, 12, 192, 3, layout))            # TT = 2, short last tile of 1
        out.append(("f32", 2, 1, 12, 192, 3, layout))            # TT = 2, T < TT
        out.append(("f32", 1, 3, 12, 384, 3, layout))            # TT = 1
    out.append(("f32", 1, 257, 16, 160, 3, "packed"))            # ViT-H
    out.append(("bf16", 1, 257, 16, 160, 3, "packed_ld"))
    have = heads_reached(out)
    for key, (c, H, n_s) in sorted(heads_reachable().items()):
        if key not in have:
            r = heads_route(key[0], c, H, n_s, key[2])
            if r[3] > 64 * 1024:
                continue                                          # the opt-in LDS path has a test (and a case list) of its own: below
            out.append((key[0], 1, HEADS_T[k % 5], H, c, n_s, LAYOUTS[k % 4]))
            k += 1
            have = heads_reached(out)
    return out


def heads_reached(cs):
    got = {}
    for case in cs:
        dtype, B, T, H, c, n_s, layout = case
        for d in (0, 1):
            r = heads_route(dtype, c, H, n_s, d)
            if r[0] != "refused":
                got.setdefault((dtype, r[0], d, r[1]), case)
    return got


def heads_big_lds_cases():
    """A token row of 67 584 B (TT = 1 and the opt-in LDS size), then the smallest shape of every instantiation that only a
    tile above 64 KiB selects."""
    out = [("f32", 1, 2, 8, 704, 3, "packed")]
    have = heads_reached(heads_cases() + out)
    for key, (c, H, n_s) in sorted(heads_reachable().items()):
        if key not in have:
            out.append((key[0], 1, 2, H, c, n_s, LAYOUTS[len(out) % 4]))
            have = heads_reached(heads_cases() + out)
    return out


# OCTIC_ESHAPE without a launch: (dtype, B, T, H, c, n_s, direction, why)
HEADS_REFUSED = [("bf16", 1, 3, 8, 264, 3, 0, "slots"), ("f32", 1, 3, 8, 264, 1, 0, "slots"), ("f32", 1, 1, 8, 1712, 3, 0, "lds"),
                 ("f32", 1, 1, 8, 1712, 3, 1, "lds")]


def heads_view_data(dtype, B, T, c, n_s):
    """packed [B*T, 8 n_s c] of the dtype; every element of a row distinct where the format allows (a permutation test)."""
    n = 8 * n_s * c
    x = torch.randn(B * T, n, generator=gen(f"ew.heads.{dtype}.{B}.{T}.{c}.{n_s}"))
    x = x + (torch.arange(n, dtype=torch.float32) % 251)[None] * 0.0625
    return x.to(DT[dtype])


def heads_case_data(dtype, B, T, H, c, n_s):
    """(x packed [B*T, 8 n_s c], heads: n_s tensors [B, H, T, 8w]) that the oracle maps onto each other.  n_s = 3 starts from
    the view and applies pack_heads; n_s = 1 starts from the head array and applies unpack_heads (the oracle has no single
    tensor pack): a permutation is pinned from either side."""
    if n_s == 3:
        x = heads_view_data(dtype, B, T, c, 3)
        return x, heads_pack_ref(x, B, T, H, c)
    h = heads_view_data(dtype, B * H, T, c // H, 1).reshape(B, H, T, 8 * (c // H))
    return heads_unpack_ref(h), [h]


def heads_pack_ref(x, B, T, H, c):
    """n_s = 3: the oracle's pack_heads of the packed view [B*T, 24c] -> three [B, H, T, 8w]."""
    return [t.contiguous() for t in R.pack_heads(unpack5(x.reshape(B, T, -1), 3 * c), H)]


def heads_unpack_ref(h):
    """n_s = 1: the oracle's unpack_heads of [B, H, T, 8w] -> packed [B*T, 8c]."""
    xs = R.unpack_heads(h)
    return torch.cat([xs[0], xs[1], xs[2], xs[3], xs[4].flatten(-2)], dim=-1).flatten(0, 1).contiguous()


# -------------------------------------------------------------------------------------------------------- 3. D8-GELU
GELU_C = [8, 24, 160]
GELU_M = [1, 5, 34]                  # 34 = 2 samples of 17 rows
MASKS = ["all_kept", "all_dropped", "first_only", "last_only", "alternating"]
# the smallest shapes where a thread takes a second grid-stride item: (dtype, c, rps, B); M c / 4 (bf16), M c / 8 (f32) > 2^20
GELU_LARGE = [("bf16", 640, 257, 26), ("f32", 640, 257, 52)]
LARGE_MASKS = ["last_dropped", "last_kept", "alternating"]
CAST_LARGE = (160, 6682)


def mask_factors(kind, B):
    """[B] f32 sample factors: 0 = dropped, a non-power-of-two survivor scale otherwise."""
    keep = {"all_kept": [True] * B, "all_dropped": [False] * B, "first_only": [i == 0 for i in range(B)],
            "last_only": [i == B - 1 for i in range(B)], "alternating": [i % 2 == 0 for i in range(B)],
            "last_dropped": [i != B - 1 for i in range(B)], "last_kept": [i == B - 1 for i in range(B)]}[kind]
    return torch.tensor([1.0 / 0.9 if k else 0.0 for k in keep], dtype=torch.float32)


def gelu_inputs(M, c, dtype):
    """(x, g) packed [M, 8c] f32 holding values of `dtype` exactly.  Rows 1, 5, 9, ... of x are stretched to |x| <= 8 (the tails
    of erff and __expf), row 2 is exact zeros."""
    x = pack5(cases.tuple5(f"ew.gelu.x.{M}.{c}", 1, M, c, False))
    g = pack5(cases.tuple5(f"ew.gelu.g.{M}.{c}", 1, M, c, False))
    x[1::4] = (x[1::4] * 3.0).clamp(-8.0, 8.0)
    if M > 2:
        x[2] = 0.0
    return x.to(DT[dtype]).float(), g.to(DT[dtype]).float()


def gelu_oracle(x, g, c, dtype=torch.float64):
    """(y, gin) packed, of the oracle's TritonGeluD8 and its autograd evaluated in `dtype` on the device of x."""
    xs = [t.clone().requires_grad_(True) for t in unpack5(x.to(dtype)[None], c)]
    ys = R.TritonGeluD8()(tuple(xs))
    torch.autograd.backward(ys, [t.contiguous() for t in unpack5(g.to(dtype)[None], c)])
    return pack5([t.detach() for t in ys]), pack5([t.grad for t in xs])


def group_scale(ref, c):
    """max |ref| over the eight isotypic components of each (row, channel), broadcast back to [M, 8c]."""
    ref = np.abs(np.asarray(ref, np.float64))
    M = ref.shape[0]
    return np.broadcast_to(ref.reshape(M, 8, c).max(1, keepdims=True), (M, 8, c)).reshape(M, 8 * c)


def scaled_err(got, ref, scale):
    """max |got - ref| / scale; where the scale is 0 the difference must be 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / scale, np.where(d > 0, np.inf, 0.0))
    return float(np.nan_to_num(e, nan=np.inf).max()) if e.size else 0.0


@functools.lru_cache(maxsize=None)
def gelu_case(M, c, dtype):
    x, g = gelu_inputs(M, c, dtype)
    y, gin = (t.numpy() for t in gelu_oracle(x, g, c))
    y32, gin32 = (t.numpy() for t in gelu_oracle(x, g, c, torch.float32))
    return dict(x=x, g=g, y=y, gin=gin, oracle_y=scaled_err(y32, y, group_scale(y, c)),
                oracle_gin=scaled_err(gin32, gin, group_scale(gin, c)))


# ------------------------------------------------------------------------------------------------ 4. the small kernels
SMALL_C = [8, 24, 160]
CAST_RPS = [1, 17]
CAST_M = 34                          # 34 c chunks of 8: no multiple of 256 at any c of SMALL_C
COLSUM_C = [8, 48, 1024]             # 128 row lanes; c4 = 12, four idle threads; one lane
COLSUM_M = [1, 127, 128, 129, 2049]  # partial blocks of 128 rows: 1 block .. 17 blocks (the finish kernel has 16 block lanes)
IM2COL = [(2 * 14, 3 * 14, 14), (3 * 16, 2 * 16, 16)]      # (Himg, Wimg, p): 2 x 3 and 3 x 2 patches


def small_x(tag, M, c):
    return pack5(cases.tuple5(f"ew.{tag}.{M}.{c}", 1, M, c))


def cast_scales(B):
    """0 first (signed zeros), then factors that are no powers of two."""
    return torch.tensor([0.0] + [1.0 / 0.9 - 0.37 * i for i in range(1, B)], dtype=torch.float32)


def spectrum_x(M, c):
    """packed f32 [M, 8c] with exact zeros, -0.0 and E pairs a = b = 0 (and a = 0 alone, b = 0 alone) at fixed places."""
    x = small_x("ps", M, c)
    j = torch.arange(c)
    for k in (1, 2, 3):
        x[:, k * c + (j[j % 5 == 0])] = 0.0
        x[:, k * c + (j[j % 5 == 1])] = -0.0
    e0, e1 = x[:, 4 * c:6 * c], x[:, 6 * c:8 * c]
    j2 = torch.arange(2 * c)
    e0[:, j2[j2 % 7 == 0]] = 0.0
    e1[:, j2[j2 % 7 == 0]] = 0.0
    e0[:, j2[j2 % 7 == 1]] = -0.0
    e1[:, j2[j2 % 7 == 1]] = 0.0
    e0[:, j2[j2 % 7 == 2]] = 0.0       # a = 0 alone
    e1[:, j2[j2 % 7 == 3]] = -0.0      # b = -0 alone
    return x


def spectrum_oracle(x, dd, c, dtype=torch.float64):
    """(invariant [M, 6c], dx packed [M, 8c]) of the oracle's PowerSpectrumInvariant and its autograd in `dtype`."""
    xs = [t.clone().requires_grad_(True) for t in unpack5(x.to(dtype)[None], c)]
    y = R.PowerSpectrumInvariant(8 * c)(tuple(xs))
    y.backward(dd.to(dtype)[None])
    return y.detach()[0], pack5([t.grad for t in xs])


def spectrum_grad_scale(dx, c):
    """per element of the packed gradient: |ref| for the one-dimensional irreps, max(|da|, |db|) of the pair for E."""
    s = np.abs(np.asarray(dx, np.float64)).copy()
    pair = np.maximum(s[:, 4 * c:6 * c], s[:, 6 * c:8 * c])
    s[:, 4 * c:6 * c] = pair
    s[:, 6 * c:8 * c] = pair
    return s


@functools.lru_cache(maxsize=None)
def spectrum_case(M, c):
    x = spectrum_x(M, c)
    dd = torch.randn(M, 6 * c, generator=gen(f"ew.ps.dd.{M}.{c}"))
    y, dx = (t.numpy() for t in spectrum_oracle(x, dd, c))
    y32, dx32 = (t.numpy() for t in spectrum_oracle(x, dd, c, torch.float32))
    return dict(x=x, dd=dd, y=y, dx=dx, oracle_y=scaled_err(y32, y, np.abs(y)),
                oracle_dx=scaled_err(dx32, dx, spectrum_grad_scale(dx, c)))


def im2col_ref(img, p, Kpad):
    """[B, Cin, H, W] -> [B Gh Gw, Kpad]: row = (b, gy, gx), column = (ch, py, px), the pad columns 0."""
    B, Cin, Himg, Wimg = img.shape
    Gh, Gw = Himg // p, Wimg // p
    t = img.reshape(B, Cin, Gh, p, Gw, p).permute(0, 2, 4, 1, 3, 5).reshape(B * Gh * Gw, Cin * p * p)
    out = torch.zeros(B * Gh * Gw, Kpad)
    out[:, :Cin * p * p] = t
    return out


def int_matrix(tag, M, c):
    """integers in [-8, 8]: exact in bf16 and f32, and so is every column sum of up to 2^20 rows"""
    return torch.randint(-8, 9, (M, c), generator=gen(f"ew.int.{tag}.{M}.{c}")).float()
