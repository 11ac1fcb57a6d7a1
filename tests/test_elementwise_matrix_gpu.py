"""Every kernel instance of csrc/elementwise.hip through the C ABI (ctypes), at every instantiation, layout and edge, against
the references of tests/golden/elementwise_cases.py.

Checks
  exact     the weight preparations, head pack / unpack, cast_rowscale, handoff_cat, im2col and colsum_a1 (integer operands)
            are one rounding or none: torch.equal on the bits against torch on the CPU.
  GELU      reference: the oracle's TritonGeluD8 in float64 with autograd, on the kernel's own (already rounded) inputs.  The
            error of an element is divided by the max |reference| over the eight isotypic components of its (row, channel):
            the butterflies mix exactly those eight.  The f32 bar of a case is 4 x the error of the same oracle evaluated in
            float32 on the CPU on the same inputs, measured the same way, with a floor of 4 * 2^-24 (both are O(eps) walks over
            about a dozen roundings that differ in association; the margin rule of the LayerNormD8 suite).  bf16 outputs:
            |got - ref64| <= 1/2 ulp_bf16(ref64) + the f32 bar * the group scale.  No term for __expf is added: the kernels
            meet the bar without one (NOTES.md has the measured table).
  spectrum  the same rule; the forward per element, the E gradient by max(|da|, |db|) of the reference pair; where the
            reference is exactly zero (zeros, -0.0, E pairs a = b = 0) the kernel's value must be zero.
  masks     rows of dropped samples are poisoned with NaN on input and must come out +0 bit for bit; kept rows are bitwise
            those of the unmasked launch.
Every operand lies in a NaN-filled arena with guard rows (and, for the *_ld layouts, gap columns and a row stride of its
own): after every launch nothing outside the documented extent may have changed, no NaN may be left inside it, and the
inputs are bitwise what they were.

The M >= 2^31 branch of RowMask (64-bit division) needs 2^31 rows of at least 64 bytes: it cannot be reached with real
memory and is not tried.

Kernel instances and the cases that run them (every instance the launchers of elementwise.hip can select):
  gelu_fwd4 / gelu_bwd4 <bf16, SKIP 0|1>       test_gelu, test_gelu_masked (bf16); second item: test_gelu_second_item[bf16]
  gelu_fwd / gelu_bwd <float, SKIP 0|1>         the same tests (f32); second item: test_gelu_second_item[f32]
  cast_rowscale <float | bf16>                  test_cast_rowscale; past the grid cap: test_cast_rowscale_past_the_grid_cap
  heads_permute <T, V, DIR, SLOTS>              all 84 instantiations are reachable (elementwise_cases.heads_reachable walks
                                                every shape heads_check accepts); test_heads runs 82 of them,
                                                test_heads_lds_above_64k the two that only a tile above 64 KiB selects
                                                (<bf16, 1, unpack, 16> at c = 4104, <float, 1, unpack, 16> at c = 2056);
                                                test_heads_table_reaches_every_instantiation prints the (T, V, DIR, SLOTS,
                                                TT) -> case table and fails on a gap
  handoff_cat <float | bf16, 0>, <float, 1>     test_handoff_cat
  power_spectrum_fwd <float | bf16>, _bwd       test_power_spectrum
  im2col <float | bf16>                         test_im2col
  colsum_partial <float | bf16>, colsum_finish  test_colsum_a1
  linear_prep <float | bf16>                    test_prep_batch_* (the per-layer launch is held to the same bits)
  linear_prep_batch <float | bf16>              test_prep_batch_one_item, _three_items, _many_items
  sample_blocks <0 | 1>                         tests/test_kernels_gpu.py test_sample_blocks_gather_and_scatter (not here)

OCTIC_EW_REPORT=<file> writes the measured kernel and oracle errors per kernel instance as JSON (the table of NOTES.md).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import elementwise_cases as E
from ln_d8_cases import pack5, unpack5
from oracle import octic_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2                       # guard rows in front of and behind every arena
F32, BF16, BAD_DTYPE = 0, 1, 7  # dtype codes of include/octic_hip.h, and one that is none
OCTIC_ESHAPE, OCTIC_EALIGN, OCTIC_EDTYPE, OCTIC_ENULL = -1, -2, -3, -4
FLOOR = 4 * 2.0 ** -24
DT = E.DT
CODE = {"f32": F32, "bf16": BF16}
REPORT = {}                     # (kernel, quantity) -> [kernel error, oracle error], maxima over the cases


# ------------------------------------------------------------------------------------------------------------- ABI
def lib():
    from octic_vits_amd import _lib
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    if t is None:
        return ctypes.c_void_p(0)
    return ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _arr(n, ptrs):
    a = (ctypes.c_void_p * n)()
    for i in range(n):
        a[i] = ptrs[i] if i < len(ptrs) and ptrs[i] else 0
    return a


def _ref(v):
    return ctypes.byref(v) if v is not None else None


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


# ---------------------------------------------------------------------------------------------------------- arenas
class Arena:
    """One allocation of GUARD + rows + GUARD rows of ld elements, NaN everywhere except where `data` goes (the first `width`
    columns of the middle rows: the extent a kernel may read or write)."""

    def __init__(self, rows, width, ld=None, dtype=torch.float32, data=None):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.buf = torch.full((rows + 2 * GUARD, self.ld), float("nan"), dtype=dtype, device=DEV)
        if data is not None:
            self.body().copy_(data.reshape(rows, width))
        self.snap = self.buf.clone()

    def body(self):
        return self.buf[GUARD:GUARD + self.rows, :self.width]

    def ptr(self, col=0):
        return self.body().data_ptr() + col * self.buf.element_size()

    def unchanged(self):
        return torch.equal(_bits(self.buf), _bits(self.snap))

    def outside_untouched(self):
        m = torch.ones(self.buf.shape, dtype=torch.bool, device=DEV)
        m[GUARD:GUARD + self.rows, :self.width] = False
        return torch.equal(_bits(self.buf)[m], _bits(self.snap)[m])

    def filled(self):
        return not bool(torch.isnan(self.body()).any())


class Feature:
    """An octic feature of M rows in one of the four memory layouts.  slot: the operand's number in its call, so that every
    operand (and every tensor of a tuple) gets a row stride of its own under the *_ld layouts."""

    def __init__(self, M, c, dtype, kind, slot, data=None):
        self.c, self.kind = c, kind
        pad = kind.endswith("_ld")
        if kind.startswith("packed"):
            spans = [(0, 8 * c)]
        else:
            spans = [(0, c), (c, c), (2 * c, c), (3 * c, c), (4 * c, 4 * c)]          # the E tensor is [M, 2, 2c]
        self.arenas = [Arena(M, w, w + (8 * (slot + i + 1) if pad else 0), dtype, None if data is None else data[:, lo:lo + w])
                       for i, (lo, w) in enumerate(spans)]

    def view(self):
        from octic_vits_amd._lib import OcticView
        v = OcticView()
        if len(self.arenas) == 1:
            a = self.arenas[0]
            for i in range(5):
                v.ptr[i] = a.ptr(i * self.c)
                v.ld[i] = a.ld
        else:
            for i, a in enumerate(self.arenas):
                v.ptr[i] = a.ptr()
                v.ld[i] = a.ld
        for i in range(5):                                   # what check_view asks of a caller
            assert v.ptr[i] % 16 == 0 and (v.ld[i] * self.arenas[0].buf.element_size()) % 16 == 0
        return v

    def packed(self):
        return torch.cat([a.body() for a in self.arenas], dim=1)

    def unchanged(self):
        return all(a.unchanged() for a in self.arenas)

    def outside_untouched(self):
        return all(a.outside_untouched() for a in self.arenas)

    def filled(self):
        return all(a.filled() for a in self.arenas)


def _io(tag, fails, inputs=(), outputs=()):
    """What holds after every launch: inputs bitwise unchanged, nothing written outside an output's extent, no NaN inside."""
    if not all(a.unchanged() for a in inputs if a is not None):
        fails.append(f"{tag}: an input changed")
    if not all(a.outside_untouched() for a in outputs if a is not None):
        fails.append(f"{tag}: a write outside an output's extent")
    if not all(a.filled() for a in outputs if a is not None):
        fails.append(f"{tag}: output elements left unwritten (or NaN)")


def _done(fails):
    for f in fails:
        print(f)
    assert not fails, f"{len(fails)} checks failed, the first: " + " | ".join(fails[:5])


def _equal(tag, fails, got, want, what):
    """bitwise; got on the device, want on the CPU"""
    got = got.contiguous().cpu()
    if not _same(got, want):
        fails.append(f"{tag}: {what} differs in {int((_bits(got) != _bits(want.contiguous())).sum())} of {want.numel()} elements")


# ------------------------------------------------------------------------------------------------------------ bars
def _bar(oracle_err):
    return max(4.0 * oracle_err, FLOOR)


def _note(kernel, quantity, got, oracle):
    r = REPORT.setdefault((kernel, quantity), [0.0, 0.0])
    r[0], r[1] = max(r[0], got), max(r[1], oracle)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("OCTIC_EW_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump([dict(kernel=k[0], quantity=k[1], kernel_err=v[0], oracle_f32_err=v[1], bar=_bar(v[1]))
                       for k, v in sorted(REPORT.items())], f, indent=1)


def _bf16_half_ulp(ref):
    """half the spacing of bfloat16 (8 significant bits) at |ref|; 0 at 0"""
    _, ex = np.frexp(np.abs(ref))
    return np.where(ref != 0, np.ldexp(0.5, ex - 8), 0.0)


def _value(tag, fails, kernel, quantity, dtype, got, ref, scale, oracle_err):
    """got against the float64 reference under the bar of the module docstring.  f32: max |got - ref| / scale <= bar.
    bf16: |got - ref| <= half an ulp of bf16 at ref + bar * scale.  What is noted is the f32 error, resp. the part of the bf16
    error beyond half an ulp, over the scale."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bar = _bar(oracle_err)
    half = _bf16_half_ulp(ref) if dtype == "bf16" else 0.0
    err = E.scaled_err(np.maximum(np.abs(got - ref) - half, 0.0), np.zeros_like(ref), scale)
    _note(kernel, quantity, err, oracle_err)
    if not err <= bar:
        fails.append(f"{tag}: {quantity} error {err:.3e} > bar {bar:.3e} (f32 oracle {oracle_err:.3e})")


# ================================================================================================ 1. weight preparation
class PrepItem:
    """One LinearD8's masters, layer scales and guarded output buffers on the device, with the expected bits."""

    def __init__(self, tag, cin, cout, dtype, cs=True, wb=True, wt=True):
        self.cin, self.cout, self.dtype = cin, cout, dtype
        self.w5, cs5 = E.prep_inputs(tag, cin, cout)
        self.cs5 = cs5 if cs else None
        self.w = [Arena(1, t.numel(), data=t) for t in self.w5]
        self.cs = [Arena(1, t.numel(), data=t) for t in cs5] if cs else None
        n = 8 * cin * cout
        self.wb = Arena(1, n, dtype=DT[dtype]) if wb else None
        self.wt = Arena(1, n, dtype=DT[dtype]) if wt else None
        self.want_wb, self.want_wt = E.prep_ref(self.w5, self.cs5, DT[dtype])
        self.blocks = lib().octic_linear_d8_prep_batch_blocks(cin, cout)
        assert self.blocks == E.prep_tiles(cin, cout)

    def row(self, tab, i, begin):
        tab[i]["w"] = [a.ptr() for a in self.w]
        tab[i]["cs"] = [a.ptr() for a in self.cs] if self.cs else [0] * 5
        tab[i]["wb"], tab[i]["wt"] = (self.wb.ptr() if self.wb else 0), (self.wt.ptr() if self.wt else 0)
        tab[i]["cin"], tab[i]["cout"], tab[i]["block_begin"], tab[i]["block_count"] = self.cin, self.cout, begin, self.blocks

    def check(self, tag, fails):
        _io(tag, fails, self.w + (self.cs or []), [self.wb, self.wt])
        if self.wb:
            _equal(tag, fails, self.wb.body()[0], self.want_wb, "wb")
        if self.wt:
            _equal(tag, fails, self.wt.body()[0], self.want_wt, "wt")

    def per_layer(self, tag, fails):
        """octic_linear_d8_prep on the same inputs: the same bits."""
        other = PrepItem.__new__(PrepItem)
        other.__dict__.update(self.__dict__)
        n = 8 * self.cin * self.cout
        other.wb = Arena(1, n, dtype=DT[self.dtype]) if self.wb else None
        other.wt = Arena(1, n, dtype=DT[self.dtype]) if self.wt else None
        rc = lib().octic_linear_d8_prep(_arr(5, [a.ptr() for a in self.w]), _arr(5, [a.ptr() for a in self.cs]) if self.cs else None,
                                        self.cin, self.cout, _p(other.wb and other.wb.ptr()), _p(other.wt and other.wt.ptr()),
                                        CODE[self.dtype], _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{tag}: octic_linear_d8_prep returned {rc}"
        other.check(tag + " per-layer launch", fails)
        for name in ("wb", "wt"):
            a, b = getattr(self, name), getattr(other, name)
            if a is not None and not _same(a.body(), b.body()):
                fails.append(f"{tag}: {name} of the batched and the per-layer launch differ")


def _prep_batch(items, dtype):
    tab = np.zeros(len(items), dtype=E.PREP_ITEM_DTYPE)
    begin = 0
    for i, it in enumerate(items):
        it.row(tab, i, begin)
        begin += it.blocks
    dev_tab = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    rc = lib().octic_linear_d8_prep_batch(_p(dev_tab), len(items), begin, CODE[dtype], _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("cin,cout", E.PREP_SHAPES)
def test_prep_batch_one_item(cin, cout, dtype):
    fails = []
    it = PrepItem("one", cin, cout, dtype)
    tag = f"prep_batch {cin}x{cout} {dtype}"
    assert _prep_batch([it], dtype) == 0
    it.check(tag, fails)
    it.per_layer(tag, fails)
    _done(fails)


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_prep_batch_three_items(dtype):
    """Three shapes in one table; one item without layer scales, one without wb, one without wt."""
    fails = []
    items = [PrepItem(f"three{i}", cin, cout, dtype, cs=i != 0, wb=i != 1, wt=i != 2) for i, (cin, cout) in enumerate(E.PREP_TABLE3)]
    assert _prep_batch(items, dtype) == 0
    for i, it in enumerate(items):
        it.check(f"prep_batch item {i} {it.cin}x{it.cout} {dtype}", fails)
        it.per_layer(f"prep_batch item {i} {it.cin}x{it.cout} {dtype}", fails)
    _done(fails)


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_prep_batch_many_items(dtype):
    """300 items of (8, 8): 1500 workgroups, and the item search of a workgroup takes its second pass of 256 items.  All
    masters in one arena (a row per item), all layer scales in a second, wb and wt in one each with gap columns between items."""
    n, cin, cout = E.PREP_MANY, 8, 8
    W = torch.randn(n, 512, generator=E.gen("ew.prep.many.w"))
    CS = 0.7 * torch.randn(n, 48, generator=E.gen("ew.prep.many.cs")) + 0.3
    wa, ca = Arena(n, 512, 520, data=W), Arena(n, 48, 56, data=CS)
    wb, wt = Arena(n, 512, 528, DT[dtype]), Arena(n, 512, 536, DT[dtype])
    tab = np.zeros(n, dtype=E.PREP_ITEM_DTYPE)
    blocks = E.prep_tiles(cin, cout)
    es = 2 if dtype == "bf16" else 4
    want_b, want_t = [], []
    for i in range(n):
        tab[i]["w"] = [wa.ptr() + 4 * (i * wa.ld + 64 * g) for g in range(5)]
        tab[i]["cs"] = [ca.ptr() + 4 * (i * ca.ld + 8 * g) for g in range(5)]
        tab[i]["wb"], tab[i]["wt"] = wb.ptr() + es * i * wb.ld, wt.ptr() + es * i * wt.ld
        tab[i]["cin"], tab[i]["cout"], tab[i]["block_begin"], tab[i]["block_count"] = cin, cout, i * blocks, blocks
        w5 = [W[i, 64 * g:64 * g + 64].reshape(8, 8) for g in range(4)] + [W[i, 256:].reshape(16, 16)]
        cs5 = [CS[i, 8 * g:8 * g + 8] for g in range(4)] + [CS[i, 32:]]
        b, t = E.prep_ref(w5, cs5, DT[dtype])
        want_b.append(b)
        want_t.append(t)
    dev_tab = torch.from_numpy(tab.view(np.uint8).copy()).to(DEV)
    assert n * blocks == 1500
    assert lib().octic_linear_d8_prep_batch(_p(dev_tab), n, n * blocks, CODE[dtype], _stream()) == 0
    torch.cuda.synchronize()
    fails = []
    _io(f"prep_batch 300 items {dtype}", fails, [wa, ca], [wb, wt])
    _equal(f"prep_batch 300 items {dtype}", fails, wb.body(), torch.stack(want_b), "wb")
    _equal(f"prep_batch 300 items {dtype}", fails, wt.body(), torch.stack(want_t), "wt")
    _done(fails)


# ================================================================================================ 2. head pack / unpack
def _run_heads(case, fails):
    dtype, B, T, H, c, n_s, layout = case
    M, hd = B * T, 8 * (c // H)
    tag = f"heads {dtype} B={B} T={T} H={H} c={c} n_s={n_s} {layout}"
    x, heads = E.heads_case_data(dtype, B, T, H, c, n_s)
    xf = Feature(M, n_s * c, DT[dtype], layout, 0, x)
    ha = [Arena(1, B * H * T * hd, dtype=DT[dtype]) for _ in range(n_s)]
    xv = xf.view()
    rc = lib().octic_attn_pack_heads(_ref(xv), _arr(3, [a.ptr() for a in ha]), B, T, H, c, n_s, CODE[dtype], _stream())
    torch.cuda.synchronize()
    if E.heads_route(dtype, c, H, n_s, 0)[0] == "refused":       # a shape chosen for its unpack instantiation: more than 16 pack slots
        if rc != OCTIC_ESHAPE or not (xf.unchanged() and all(a.unchanged() for a in ha)):
            fails.append(f"{tag}: pack returned {rc} for a shape it refuses, or moved a byte")
    elif rc != 0:
        fails.append(f"{tag}: pack returned {rc}")
        return
    else:
        _io(tag + " pack", fails, [xf], ha)
        for s in range(n_s):
            _equal(tag + " pack", fails, ha[s].body()[0], heads[s].flatten(), f"heads[{s}]")
    # unpack reads what the oracle packed (so it does not lean on the launch above)
    hb = [Arena(1, B * H * T * hd, dtype=DT[dtype], data=h) for h in heads]
    yf = Feature(M, n_s * c, DT[dtype], layout, 1)
    yv = yf.view()
    rc = lib().octic_attn_unpack_heads(_arr(3, [a.ptr() for a in hb]), _ref(yv), B, T, H, c, n_s, CODE[dtype], _stream())
    torch.cuda.synchronize()
    assert E.heads_route(dtype, c, H, n_s, 1)[0] != "refused"    # (a pack goes through fewer elements per access: never the other way)
    if rc != 0:
        fails.append(f"{tag}: unpack returned {rc}")
        return
    _io(tag + " unpack", fails, hb, [yf])
    _equal(tag + " unpack", fails, yf.packed(), x, "the view")


HEADS_CASES = E.heads_cases()


@pytest.mark.parametrize("chunk", range(0, len(HEADS_CASES), 16))
def test_heads(chunk):
    """pack against the oracle's pack_heads and unpack against its unpack_heads, bit for bit; with both exact, unpack of pack is
    the input bit for bit."""
    fails = []
    for case in HEADS_CASES[chunk:chunk + 16]:
        _run_heads(case, fails)
    _done(fails)


def test_heads_lds_above_64k():
    """A tile above 64 KiB of LDS: the launch opts in to the larger dynamic size first (160 KiB per CU on this device)."""
    fails = []
    for case in E.heads_big_lds_cases():
        dtype, B, T, H, c, n_s, layout = case
        r = E.heads_route(dtype, c, H, n_s, 1)                        # (TT and the tile size are those of the pack direction too)
        assert r[2] == 1 and 64 * 1024 < r[3] <= E.HEADS_MAX_LDS, (case, r)
        _run_heads(case, fails)
    _done(fails)


def test_heads_table_reaches_every_instantiation():
    """(T, V, DIR, SLOTS) of every case from the formulas of heads_launch / heads_dispatch: the tables reach every
    instantiation a shape can select, the named ones as intended, TT = 4, 2 and 1, and the token counts asked for."""
    reach = E.heads_reachable()
    got = E.heads_reached(HEADS_CASES + E.heads_big_lds_cases())
    for key in sorted(reach):
        case = got.get(key)
        print(f"heads_permute<{key[0]}, V={key[1]}, DIR={key[2]}, SLOTS={key[3]}>  <-  {case}"
              + (f"  TT={E.heads_route(case[0], case[4], case[3], case[5], key[2])[2]}" if case else ""))
    assert not [k for k in reach if k not in got]
    assert not [k for k in E.heads_all_instances() if k not in reach], "an instantiation no shape selects: name it in the docstring"
    R_ = lambda dt, c, H, n_s, d: E.heads_route(dt, c, H, n_s, d)[:3]
    assert R_("bf16", 72, 8, 3, 0) == (1, 5, 4) and R_("bf16", 120, 8, 1, 0) == (1, 8, 4) and R_("bf16", 136, 8, 3, 0) == (1, 16, 4)
    assert R_("f32", 192, 12, 3, 0)[2] == 2 and R_("f32", 384, 12, 3, 1)[2] == 1
    tts = {E.heads_route(cs[0], cs[4], cs[3], cs[5], 1)[2] for cs in HEADS_CASES}
    assert tts == {1, 2, 4}
    assert {cs[2] for cs in HEADS_CASES} == {1, 3, 4, 5, 7, 257}
    assert {(cs[5], cs[6]) for cs in HEADS_CASES} == {(n, l) for n in (1, 3) for l in E.LAYOUTS}


@pytest.mark.parametrize("dtype,B,T,H,c,n_s,direction,why", E.HEADS_REFUSED)
def test_heads_refuses_without_a_launch(dtype, B, T, H, c, n_s, direction, why):
    """More than 16 slots, or a single token row above 160 KiB: OCTIC_ESHAPE, and not a byte moves."""
    assert E.heads_route(dtype, c, H, n_s, direction) == ("refused", why)
    M, hd = B * T, 8 * (c // H)
    xf = Feature(M, n_s * c, DT[dtype], "packed", 0, E.heads_view_data(dtype, B, T, c, n_s))
    ha = [Arena(1, B * H * T * hd, dtype=DT[dtype]) for _ in range(n_s)]
    xv = xf.view()
    hp = _arr(3, [a.ptr() for a in ha])
    if direction == 0:
        rc = lib().octic_attn_pack_heads(_ref(xv), hp, B, T, H, c, n_s, CODE[dtype], _stream())
    else:
        rc = lib().octic_attn_unpack_heads(hp, _ref(xv), B, T, H, c, n_s, CODE[dtype], _stream())
    torch.cuda.synchronize()
    assert rc == OCTIC_ESHAPE
    assert xf.unchanged() and all(a.unchanged() for a in ha)


# ============================================================================================================ 3. D8-GELU
GELU_KERNEL = {"bf16": ("gelu_fwd4<bf16>", "gelu_bwd4<bf16>"), "f32": ("gelu_fwd<float>", "gelu_bwd<float>")}


def _launch_gelu(x, g, M, c, dtype, layout, ss=None, rps=0, always_skip_entry=False):
    """forward and backward launch on packed [M, 8c] data; returns (rc fwd, rc bwd, x, g, y, gin Features)."""
    xf, gf = Feature(M, c, DT[dtype], layout, 0, x), Feature(M, c, DT[dtype], layout, 1, g)
    yf, of = Feature(M, c, DT[dtype], layout, 2), Feature(M, c, DT[dtype], layout, 3)
    xv, gv, yv, ov = xf.view(), gf.view(), yf.view(), of.view()
    if ss is None and not always_skip_entry:
        r1 = lib().octic_gelu_d8_fwd(_ref(xv), _ref(yv), M, c, CODE[dtype], _stream())
        r2 = lib().octic_gelu_d8_bwd(_ref(gv), _ref(xv), _ref(ov), M, c, CODE[dtype], _stream())
    else:
        r1 = lib().octic_gelu_d8_fwd_skip(_ref(xv), _ref(yv), M, c, CODE[dtype], _p(ss), rps, _stream())
        r2 = lib().octic_gelu_d8_bwd_skip(_ref(gv), _ref(xv), _ref(ov), M, c, CODE[dtype], _p(ss), rps, _stream())
    torch.cuda.synchronize()
    return r1, r2, xf, gf, yf, of


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.GELU_C)
def test_gelu(c, dtype, layout):
    """Forward and backward at every small row count against the float64 oracle, under the bar of the module docstring."""
    fails = []
    for M in E.GELU_M:
        ref = E.gelu_case(M, c, dtype)
        tag = f"gelu c={c} M={M} {dtype} {layout}"
        r1, r2, xf, gf, yf, of = _launch_gelu(ref["x"], ref["g"], M, c, dtype, layout)
        assert (r1, r2) == (0, 0), f"{tag}: returned {r1}, {r2}"
        _io(tag, fails, [xf, gf], [yf, of])
        _value(tag, fails, GELU_KERNEL[dtype][0], "y", dtype, yf.packed().double().cpu().numpy(), ref["y"],
               E.group_scale(ref["y"], c), ref["oracle_y"])
        _value(tag, fails, GELU_KERNEL[dtype][1], "gin", dtype, of.packed().double().cpu().numpy(), ref["gin"],
               E.group_scale(ref["gin"], c), ref["oracle_gin"])
    _done(fails)


def _masked_against_plain(tag, fails, M, rps, keep_rows, plain, masked):
    """plain, masked: (y, gin) Features.  Dropped rows +0 bit for bit, kept rows bitwise those of the unmasked launch."""
    for name, a, b in zip(("y", "gin"), plain, masked):
        pa, pb = a.packed(), b.packed()
        if _bits(pb[~keep_rows]).count_nonzero().item():
            fails.append(f"{tag}: {name} of a dropped sample is not +0")
        if not _same(pa[keep_rows], pb[keep_rows]):
            fails.append(f"{tag}: {name} of a kept sample differs from the unmasked launch")


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("c", E.GELU_C)
def test_gelu_masked(c, dtype, layout):
    """octic_gelu_d8_*_skip: rps 1 and 17, five masks; dropped samples' input rows are NaN."""
    fails = []
    for M, rps in ((34, 17), (34, 1), (5, 1), (1, 1)):
        ref = E.gelu_case(M, c, dtype)
        _, _, _, _, y0, o0 = _launch_gelu(ref["x"], ref["g"], M, c, dtype, layout)
        B = M // rps
        for kind in E.MASKS:
            tag = f"gelu masked c={c} M={M} rps={rps} {kind} {dtype} {layout}"
            ss = E.mask_factors(kind, B)
            keep = (ss != 0).repeat_interleave(rps)
            x, g = ref["x"].clone(), ref["g"].clone()
            x[~keep] = float("nan")
            g[~keep] = float("nan")
            r1, r2, xf, gf, yf, of = _launch_gelu(x, g, M, c, dtype, layout, ss.to(DEV), rps)
            assert (r1, r2) == (0, 0), f"{tag}: returned {r1}, {r2}"
            _io(tag, fails, [xf, gf], [yf, of])
            _masked_against_plain(tag, fails, M, rps, keep.to(DEV), (y0, o0), (yf, of))
    _done(fails)


@pytest.mark.parametrize("dtype,c,rps,B", E.GELU_LARGE)
def test_gelu_second_item(dtype, c, rps, B):
    """The smallest shape where a thread takes a second grid-stride item (the grid is capped at 4096 blocks).  The second
    items lie in the last sample, the first items of the same threads in the first: the masks give the two samples opposite
    states, which the masked kernels' one-item look-ahead must carry.  Values on every 97th row and the last 300 rows."""
    M = B * rps
    per = 4 if dtype == "bf16" else 8
    assert E.second_item(M * c // per) and not E.second_item((M - rps) * c // per)
    first_second = E.GRID_CAP * 256 * per // c                                 # the row of the first second item
    assert first_second // rps == B - 1 and (M * c // per - E.GRID_CAP * 256) * per // c < rps
    gen = torch.Generator(device=DEV).manual_seed(20 + B)
    x = torch.randn(M, 8 * c, generator=gen, device=DEV)
    x[1::4] = (x[1::4] * 3.0).clamp(-8.0, 8.0)
    x[2] = 0.0
    x = x.to(DT[dtype]).float()
    g = torch.randn(M, 8 * c, generator=gen, device=DEV).to(DT[dtype]).float()
    fails = []
    tag = f"gelu second item {dtype} c={c} M={M}"
    r1, r2, xf, gf, y0, o0 = _launch_gelu(x, g, M, c, dtype, "packed")
    assert (r1, r2) == (0, 0)
    _io(tag, fails, [xf, gf], [y0, o0])
    rows = torch.unique(torch.cat([torch.arange(0, M, 97), torch.arange(M - 300, M)])).to(DEV)
    xs, gs = x[rows], g[rows]
    y64, g64 = (t.cpu().numpy() for t in E.gelu_oracle(xs, gs, c))             # float64 on the device
    y32, g32 = (t.numpy() for t in E.gelu_oracle(xs.cpu(), gs.cpu(), c, torch.float32))
    for kern, q, got, r64, r32 in ((0, "y", y0, y64, y32), (1, "gin", o0, g64, g32)):
        scale = E.group_scale(r64, c)
        _value(tag, fails, GELU_KERNEL[dtype][kern] + " second item", q, dtype, got.packed()[rows].double().cpu().numpy(), r64, scale,
               E.scaled_err(r32, r64, scale))
    for kind in E.LARGE_MASKS:
        ss = E.mask_factors(kind, B).to(DEV)
        keep = (ss != 0).repeat_interleave(rps)
        xm, gm = x.clone(), g.clone()
        xm[~keep] = float("nan")
        gm[~keep] = float("nan")
        r1, r2, xf, gf, yf, of = _launch_gelu(xm, gm, M, c, dtype, "packed", ss, rps)
        assert (r1, r2) == (0, 0)
        _io(f"{tag} {kind}", fails, [xf, gf], [yf, of])
        _masked_against_plain(f"{tag} {kind}", fails, M, rps, keep, (y0, o0), (yf, of))
    _done(fails)


# ================================================================================================= 4. the small kernels
@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("c", E.SMALL_C)
def test_cast_rowscale(c, layout):
    """y = (x * rs[row // rps]).to(T) bit for bit: rs with a zero (the signed zeros torch gives) and factors that are no powers
    of two, rs = NULL, rps 1 and 17, both output dtypes."""
    M = E.CAST_M
    assert (M * c) % 256 != 0
    x = E.small_x("cast", M, c)
    fails = []
    for out in E.DTYPES:
        for rps in E.CAST_RPS + [None]:
            rs = E.cast_scales((M + rps - 1) // rps) if rps else None
            want = (x * rs.repeat_interleave(rps)[:M, None] if rps else x).to(DT[out])
            tag = f"cast_rowscale c={c} rps={rps} {out} {layout}"
            xf, yf = Feature(M, c, torch.float32, layout, 0, x), Feature(M, c, DT[out], layout, 1)
            xv, yv = xf.view(), yf.view()
            rs_d = rs.to(DEV) if rps else None
            rc = lib().octic_cast_rowscale(_ref(xv), _ref(yv), _p(rs_d), rps or 1, M, c, CODE[out], _stream())
            torch.cuda.synchronize()
            assert rc == 0, f"{tag}: returned {rc}"
            _io(tag, fails, [xf], [yf])
            _equal(tag, fails, yf.packed(), want, "y")
    _done(fails)


@pytest.mark.parametrize("out", E.DTYPES)
def test_cast_rowscale_past_the_grid_cap(out):
    c, M = E.CAST_LARGE
    assert E.second_item(M * c)
    rps, B = 257, M // 257
    x = torch.randn(M, 8 * c, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV)
    rs = E.cast_scales(B).to(DEV)
    xf, yf = Feature(M, c, torch.float32, "packed", 0, x), Feature(M, c, DT[out], "packed_ld", 1)
    xv, yv = xf.view(), yf.view()
    assert lib().octic_cast_rowscale(_ref(xv), _ref(yv), _p(rs), rps, M, c, CODE[out], _stream()) == 0
    torch.cuda.synchronize()
    fails = []
    _io("cast past the cap", fails, [xf], [yf])
    _equal("cast past the cap", fails, yf.packed(), (x.cpu() * rs.cpu().repeat_interleave(rps)[:, None]).to(DT[out]), "y")
    _done(fails)


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("c", E.SMALL_C)
def test_handoff_cat(c, layout):
    """The 5-tuple -> 8-tuple concatenation and its adjoint against convert_5tuple_to_8tuple and autograd: permutations, so
    bit for bit (and one rounding for the bf16 output)."""
    M = 19
    x = E.small_x("hand", M, c)
    xs = [t.clone().requires_grad_(True) for t in unpack5(x[None], c)]
    dense = torch.cat(R.convert_5tuple_to_8tuple(tuple(xs)), dim=-1)
    dd = torch.randn(M, 8 * c, generator=E.gen(f"ew.hand.dd.{c}"))
    dense.backward(dd[None])
    want_dx = pack5([t.grad for t in xs])
    fails = []
    for out in E.DTYPES:
        tag = f"handoff_cat_fwd c={c} {out} {layout}"
        xf, da = Feature(M, c, torch.float32, layout, 0, x), Arena(M, 8 * c, dtype=DT[out])
        xv = xf.view()
        rc = lib().octic_handoff_cat_fwd(_ref(xv), _p(da.ptr()), M, c, CODE[out], _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{tag}: returned {rc}"
        _io(tag, fails, [xf], [da])
        _equal(tag, fails, da.body(), dense.detach()[0].to(DT[out]), "dense")
    tag = f"handoff_cat_bwd c={c} {layout}"
    dda, df = Arena(M, 8 * c, data=dd), Feature(M, c, torch.float32, layout, 1)
    dv = df.view()
    rc = lib().octic_handoff_cat_bwd(_p(dda.ptr()), _ref(dv), M, c, _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{tag}: returned {rc}"
    _io(tag, fails, [dda], [df])
    _equal(tag, fails, df.packed(), want_dx, "dx")
    _done(fails)


@pytest.mark.parametrize("layout", E.LAYOUTS)
@pytest.mark.parametrize("c", E.SMALL_C)
def test_power_spectrum(c, layout):
    """Forward (f32 and bf16 output) and backward against PowerSpectrumInvariant in float64; exact zeros wherever autograd
    gives them (zeros and -0.0 in A2 / B1 / B2, E pairs a = b = 0)."""
    M = 19
    ref = E.spectrum_case(M, c)
    x = ref["x"]
    fails = []
    for out in E.DTYPES:
        tag = f"power_spectrum_fwd c={c} {out} {layout}"
        xf, da = Feature(M, c, torch.float32, layout, 0, x), Arena(M, 6 * c, dtype=DT[out])
        xv = xf.view()
        rc = lib().octic_power_spectrum_fwd(_ref(xv), _p(da.ptr()), M, c, CODE[out], _stream())
        torch.cuda.synchronize()
        assert rc == 0, f"{tag}: returned {rc}"
        _io(tag, fails, [xf], [da])
        _value(tag, fails, f"power_spectrum_fwd<{'float' if out == 'f32' else 'bf16'}>", "invariant", out,
               da.body().double().cpu().numpy(), ref["y"], np.abs(ref["y"]), ref["oracle_y"])
    tag = f"power_spectrum_bwd c={c} {layout}"
    xf, dda = Feature(M, c, torch.float32, layout, 0, x), Arena(M, 6 * c, data=ref["dd"])
    df = Feature(M, c, torch.float32, layout, 1)
    xv, dv = xf.view(), df.view()
    rc = lib().octic_power_spectrum_bwd(_p(dda.ptr()), _ref(xv), _ref(dv), M, c, _stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{tag}: returned {rc}"
    _io(tag, fails, [xf, dda], [df])
    got = df.packed().double().cpu().numpy()
    _value(tag, fails, "power_spectrum_bwd", "dx", "f32", got, ref["dx"], E.spectrum_grad_scale(ref["dx"], c), ref["oracle_dx"])
    xz = x.numpy()
    pair0 = (xz[:, 4 * c:6 * c] == 0) & (xz[:, 6 * c:8 * c] == 0)
    zero = np.concatenate([np.zeros((M, c), bool), xz[:, c:4 * c] == 0, pair0, pair0], 1)
    assert zero[:, c:4 * c].any() and pair0.any() and np.signbit(xz[zero]).any()
    if (got[zero] != 0).any():
        fails.append(f"{tag}: a gradient where the input (pair) is zero is not zero")
    _done(fails)


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("Himg,Wimg,p", E.IM2COL)
def test_im2col(Himg, Wimg, p, dtype):
    """Rectangular images (Gh != Gw), Cin 1 and 3, B 1 and 3, Kpad = K and K + pad with the pad columns exactly zero."""
    fails = []
    for Cin in (1, 3):
        for B in (1, 3):
            K = Cin * p * p
            for Kpad in sorted({(K + 7) // 8 * 8, (K + 7) // 8 * 8 + 16}):
                tag = f"im2col {Himg}x{Wimg} p={p} Cin={Cin} B={B} Kpad={Kpad} {dtype}"
                img = torch.randn(B, Cin, Himg, Wimg, generator=E.gen(f"ew.img.{Himg}.{Cin}.{B}"))
                rows = B * (Himg // p) * (Wimg // p)
                ia, pa = Arena(B * Cin * Himg, Wimg, data=img), Arena(rows, Kpad, dtype=DT[dtype])
                rc = lib().octic_im2col_patches(_p(ia.ptr()), _p(pa.ptr()), B, Cin, Himg, Wimg, p, Kpad, CODE[dtype], _stream())
                torch.cuda.synchronize()
                assert rc == 0, f"{tag}: returned {rc}"
                _io(tag, fails, [ia], [pa])
                _equal(tag, fails, pa.body(), E.im2col_ref(img, p, Kpad).to(DT[dtype]), "patches")
    _done(fails)


def _colsum(M, c, dtype, layout):
    x = E.int_matrix(f"{dtype}", M, 8 * c)
    xf = Feature(M, c, DT[dtype], layout, 0, x)
    nblk = lib().octic_colsum_blocks(M)
    assert nblk == (M + 127) // 128
    part, out = Arena(nblk, c), Arena(1, c)
    xv = xf.view()
    rc = lib().octic_colsum_a1(_ref(xv), M, c, CODE[dtype], _p(part.ptr()), _p(out.ptr()), _stream())
    torch.cuda.synchronize()
    return rc, x, xf, part, out


@pytest.mark.parametrize("c,dtype", [(c, d) for c in E.COLSUM_C for d in E.DTYPES] + [(12, "f32")])
def test_colsum_a1(c, dtype):
    """Integer operands in [-8, 8]: the column sums of the A1 block are exact, so bit for bit, at row counts that straddle the
    128 rows of a partial block and the 16 block lanes of the finish kernel; packed and padded row stride.  (c = 12: f32 moves
    chunks of four.)"""
    fails = []
    for M in E.COLSUM_M:
        for layout in ("packed", "packed_ld"):
            tag = f"colsum_a1 c={c} M={M} {dtype} {layout}"
            rc, x, xf, part, out = _colsum(M, c, dtype, layout)
            assert rc == 0, f"{tag}: returned {rc}"
            _io(tag, fails, [xf], [part, out])
            _equal(tag, fails, out.body()[0], x[:, :c].double().sum(0).float(), "the column sums")
    _done(fails)


@pytest.mark.parametrize("dtype", E.DTYPES)
def test_colsum_a1_refuses_more_than_1024_columns(dtype):
    rc, _, xf, part, out = _colsum(3, 1032, dtype, "packed")
    assert rc == OCTIC_ESHAPE and part.unchanged() and out.unchanged() and xf.unchanged()


# ========================================================================================================= argument checks
class _Args:
    """A valid small call (c = 8, M = 4, f32 or the entry's dtype) whose operands all lie in zero-filled arenas big enough for
    c = 16, and one thing wrong with it.  `wrong`: (kind, operand name); a view or buffer asked for by that name comes back NULL,
    misaligned by 4 bytes, or (views) with a row stride that breaks the 16 bytes."""

    def __init__(self, wrong=(None, None), **over):
        self.c, self.M, self.dt, self.rps = 8, 4, F32, 2
        self.__dict__.update(over)
        self.wrong, self.keep = wrong, []

    def _arena(self):
        a = Arena(8, 8 * 16 * 3, dtype=torch.float32, data=torch.zeros(8, 8 * 16 * 3))
        self.keep.append(a)
        return a

    def v(self, name):
        from octic_vits_amd._lib import OcticView
        kind, who = self.wrong
        if who == name and kind == "null_view":
            return None
        a, view = self._arena(), OcticView()
        for i in range(5):
            view.ptr[i] = a.ptr(i * 16 * 3)
            view.ld[i] = a.ld
        if who == name and kind == "null_ptr":
            view.ptr[3] = 0
        if who == name and kind == "misaligned":
            view.ptr[2] += 4
        if who == name and kind == "stride":
            view.ld[4] += 1
        self.keep.append(view)
        return ctypes.byref(view)

    def p(self, name):
        kind, who = self.wrong
        if who == name and kind == "null_ptr":
            return ctypes.c_void_p(0)
        return ctypes.c_void_p(self._arena().ptr() + (4 if who == name and kind == "misaligned" else 0))

    def untouched(self):
        return all(a.unchanged() for a in self.keep if isinstance(a, Arena))


def _heads_call(fn):
    def call(a):
        hp = (ctypes.c_void_p * 3)()
        for i in range(3):
            hp[i] = a.p(f"heads{i}").value or 0
        a.keep.append(hp)
        heads = None if a.wrong == ("null_ptr", "heads") else hp
        args = (heads, a.v("view")) if fn == "octic_attn_unpack_heads" else (a.v("view"), heads)
        return getattr(lib(), fn)(*args, 1, a.M, getattr(a, "H", 2), a.c, getattr(a, "n_s", 3), a.dt, _stream())
    return call


def _prep_call(a):
    w = _arr(5, [a.p(f"w{i}").value for i in range(5)])
    cs = _arr(5, [a.p(f"cs{i}").value for i in range(5)])
    return lib().octic_linear_d8_prep(None if a.wrong == ("null_ptr", "w") else w, cs, getattr(a, "cin", 8), 8, a.p("wb"), a.p("wt"), a.dt,
                                      _stream())


ENTRIES = {
    "octic_gelu_d8_fwd": lambda a: lib().octic_gelu_d8_fwd(a.v("x"), a.v("y"), a.M, a.c, a.dt, _stream()),
    "octic_gelu_d8_bwd": lambda a: lib().octic_gelu_d8_bwd(a.v("g"), a.v("x"), a.v("gin"), a.M, a.c, a.dt, _stream()),
    "octic_gelu_d8_fwd_skip": lambda a: lib().octic_gelu_d8_fwd_skip(a.v("x"), a.v("y"), a.M, a.c, a.dt, a.p("ss"), a.rps, _stream()),
    "octic_gelu_d8_bwd_skip": lambda a: lib().octic_gelu_d8_bwd_skip(a.v("g"), a.v("x"), a.v("gin"), a.M, a.c, a.dt, a.p("ss"), a.rps,
                                                                     _stream()),
    "octic_cast_rowscale": lambda a: lib().octic_cast_rowscale(a.v("x"), a.v("y"), a.p("rs"), a.rps, a.M, a.c, a.dt, _stream()),
    "octic_attn_pack_heads": _heads_call("octic_attn_pack_heads"),
    "octic_attn_unpack_heads": _heads_call("octic_attn_unpack_heads"),
    "octic_linear_d8_prep": _prep_call,
    "octic_linear_d8_prep_batch": lambda a: lib().octic_linear_d8_prep_batch(a.p("items"), getattr(a, "n_items", 1),
                                                                             getattr(a, "blocks", 5), a.dt, _stream()),
    "octic_handoff_cat_fwd": lambda a: lib().octic_handoff_cat_fwd(a.v("x"), a.p("dense"), a.M, a.c, a.dt, _stream()),
    "octic_handoff_cat_bwd": lambda a: lib().octic_handoff_cat_bwd(a.p("dense"), a.v("x"), a.M, a.c, _stream()),
    "octic_power_spectrum_fwd": lambda a: lib().octic_power_spectrum_fwd(a.v("x"), a.p("dense"), a.M, a.c, a.dt, _stream()),
    "octic_power_spectrum_bwd": lambda a: lib().octic_power_spectrum_bwd(a.p("dense"), a.v("x"), a.v("dx"), a.M, a.c, _stream()),
    "octic_im2col_patches": lambda a: lib().octic_im2col_patches(a.p("img"), a.p("patches"), getattr(a, "B", 1), 1, getattr(a, "Himg", 4),
                                                                 4, getattr(a, "patch", 2), getattr(a, "Kpad", 8), a.dt, _stream()),
    "octic_colsum_a1": lambda a: lib().octic_colsum_a1(a.v("x"), a.M, a.c, a.dt, a.p("partials"), a.p("out"), _stream()),
}
_VIEWS = {"octic_gelu_d8_fwd": "xy", "octic_gelu_d8_bwd": ["g", "x", "gin"], "octic_gelu_d8_fwd_skip": "xy",
          "octic_gelu_d8_bwd_skip": ["g", "x", "gin"], "octic_cast_rowscale": "xy", "octic_attn_pack_heads": ["view"],
          "octic_attn_unpack_heads": ["view"], "octic_handoff_cat_fwd": "x", "octic_handoff_cat_bwd": "x",
          "octic_power_spectrum_fwd": "x", "octic_power_spectrum_bwd": ["x", "dx"], "octic_colsum_a1": "x"}
_NULLS = {"octic_attn_pack_heads": ["heads", "heads0", "heads2"], "octic_attn_unpack_heads": ["heads", "heads1"],
          "octic_linear_d8_prep": ["w", "w0", "w4"], "octic_linear_d8_prep_batch": ["items"], "octic_handoff_cat_fwd": ["dense"],
          "octic_handoff_cat_bwd": ["dense"], "octic_power_spectrum_fwd": ["dense"], "octic_power_spectrum_bwd": ["dense"],
          "octic_im2col_patches": ["img", "patches"], "octic_colsum_a1": ["partials", "out"]}
_HAS_DTYPE = [e for e in ENTRIES if e not in ("octic_handoff_cat_bwd", "octic_power_spectrum_bwd")]


def _refusals():
    out = []
    for e in ENTRIES:
        for name in _VIEWS.get(e, ()):
            out += [(e, dict(wrong=("null_view", name)), OCTIC_ENULL), (e, dict(wrong=("null_ptr", name)), OCTIC_ENULL),
                    (e, dict(wrong=("misaligned", name)), OCTIC_EALIGN), (e, dict(wrong=("stride", name)), OCTIC_EALIGN)]
        for name in _NULLS.get(e, ()):
            out.append((e, dict(wrong=("null_ptr", name)), OCTIC_ENULL))
        if e in _VIEWS:
            out += [(e, dict(c=9), OCTIC_ESHAPE), (e, dict(c=0), OCTIC_ESHAPE), (e, dict(c=12), OCTIC_ESHAPE),
                    (e, dict(M=0), OCTIC_ESHAPE), (e, dict(M=-4), OCTIC_ESHAPE)]
        if e in _HAS_DTYPE:
            out.append((e, dict(dt=BAD_DTYPE), OCTIC_EDTYPE))
    for e in ("octic_gelu_d8_fwd_skip", "octic_gelu_d8_bwd_skip"):
        out += [(e, dict(M=5, rps=2), OCTIC_ESHAPE), (e, dict(rps=0), OCTIC_ESHAPE), (e, dict(rps=-1), OCTIC_ESHAPE)]
    out.append(("octic_cast_rowscale", dict(rps=0), OCTIC_ESHAPE))
    for e in ("octic_attn_pack_heads", "octic_attn_unpack_heads"):
        out += [(e, dict(H=3), OCTIC_ESHAPE), (e, dict(H=0), OCTIC_ESHAPE), (e, dict(n_s=2), OCTIC_ESHAPE),
                (e, dict(wrong=("misaligned", "heads1")), OCTIC_EALIGN)]
    out += [("octic_linear_d8_prep", dict(cin=0), OCTIC_ESHAPE), ("octic_linear_d8_prep_batch", dict(n_items=0), OCTIC_ESHAPE),
            ("octic_linear_d8_prep_batch", dict(blocks=0), OCTIC_ESHAPE), ("octic_im2col_patches", dict(B=0), OCTIC_ESHAPE),
            ("octic_im2col_patches", dict(Himg=5), OCTIC_ESHAPE), ("octic_im2col_patches", dict(Kpad=12), OCTIC_ESHAPE),
            ("octic_im2col_patches", dict(Kpad=0), OCTIC_ESHAPE), ("octic_im2col_patches", dict(patch=0), OCTIC_ESHAPE),
            ("octic_colsum_a1", dict(c=1032), OCTIC_ESHAPE)]
    # colsum_a1 moves 16-byte chunks of its dtype: c = 12 is a shape it takes in f32
    return [r for r in out if not (r[0] == "octic_colsum_a1" and r[1].get("c") == 12)]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_documented_refusals(entry):
    """Every refusal include/octic_hip.h documents for the entry point: the code comes back and not a byte of any operand has
    changed (nothing was launched).  The valid call of the same builder returns 0, so a refusal is the one wrong thing's."""
    good = _Args()
    if entry == "octic_linear_d8_prep_batch":                            # a valid table needs real addresses: one (8, 8) item
        it = PrepItem("args", 8, 8, "f32")
        assert _prep_batch([it], "f32") == 0
    else:
        assert ENTRIES[entry](good) == 0, "the valid call"
    torch.cuda.synchronize()
    fails = []
    for e, over, want in _refusals():
        if e != entry:
            continue
        a = _Args(**over)
        rc = ENTRIES[entry](a)
        torch.cuda.synchronize()
        if rc != want:
            fails.append(f"{entry} {over}: returned {rc}, want {want}")
        if not a.untouched():
            fails.append(f"{entry} {over}: an operand changed")
    _done(fails)
