"""PolynomialInvariant / ThirdOrderInvariant kernels (csrc/poly_invariant.hip) through the C ABI, ops, the modules and the models.

Forward: bit for bit against the stock arm (the same module with POLY_HIP off: the table-driven torch composition on the GPU) -
f32 output equal, bf16 output equal to the stock f32 output rounded once.  Rows of zeros, denormals, +-inf and NaN are planted;
NaN payloads are not compared, everything else is compared as bit patterns.
Backward, exact: small-integer operands (|x| <= 3, |g| <= 4) keep every intermediate an integer below 2^24, so dx equals the
float64 autograd of the composition bit for bit in any summation order.
Backward, random: |dx_i - dx_i^64| <= (T_i + 8) 2^-24 S_i, S_i the same sum with every sign positive at |x|, |g| in float64 and
T_i the number of monomial terms that hold x_i.  The kernel adds one rounded term per monomial that holds x_i (T_i - 1 rounded
adds from a zero accumulator) and a term is at most 3 + 1 + 1 rounded multiplies (the remaining digits, the multiplicity, the
cotangent): (1 + u)^(T_i + 4) - 1 < (T_i + 8) u for u = 2^-24 and T_i <= 24.  No factor is taken from an observed error.
Shapes: c in {8, 24, 40, 160} x M in {1, 3, 70, 257}: one item per row (c = 8 has two 4-column items), items crossing rows
inside a wave, a partial last wave and a partial last block.  The launcher does not cap its grid (one thread per item), so there
is no grid-stride loop to test; the 64-bit offsets are tested at a size whose output passes 2^31 elements.
"""
import ctypes
import functools

import pytest
import torch

from octic_vits_amd import _lib, ops
from octic_vits_amd import d8_invariantization as INV
from octic_vits_amd import functional as OF
from octic_vits_amd._lib import lib
from octic_vits_amd.d8_utils import _ISO, convert_5tuple_to_8tuple, group_elements

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
MODS = {"polynomial": INV.PolynomialInvariant, "third_order": INV.ThirdOrderInvariant}
NP = {"polynomial": 32, "third_order": 15}
# monomial terms that hold x_i, i = 0 .. 7
TERMS = {"polynomial": (1, 24, 14, 14, 23, 23, 21, 21), "third_order": (10, 4, 8, 6, 7, 7, 7, 7)}
SLOT = (0, 1, 2, 3, 4, 6, 5, 7)            # packed column block -> 8-tuple component
CS, MS = (8, 24, 40, 160), (1, 3, 70, 257)
EPS = 2.0 ** -24


def _x8(xp, c):                              # packed rows [.., 8c] -> the 8-tuple of [.., c] views
    return convert_5tuple_to_8tuple(ops.split_packed(xp, c))


def _pack8(x8):
    return torch.cat([x8[j] for j in SLOT], dim=-1)


def _count_terms(name):
    specs = ["0"] + INV._DEG2 + INV._DEG3 + INV._DEG4 if name == "polynomial" else \
        ["000"] + ["+".join("0" + t for t in s.replace("-", "+").split("+")) for s in INV._DEG2] + INV._DEG3
    terms = [t for s in specs for t in s.replace("-", "+").split("+")]
    return tuple(sum(str(i) in t for t in terms) for i in range(8))


def test_term_counts_of_the_bound_are_the_tables():
    for name in MODS:
        assert _count_terms(name) == TERMS[name]


def stock(name, xp, c):
    """The stock arm on whatever device xp lives on (the module with POLY_HIP off)."""
    old = INV.POLY_HIP
    INV.POLY_HIP = False
    try:
        return MODS[name](8 * c)(OF.Octic(xp, c))
    finally:
        INV.POLY_HIP = old


def _abs_forward(name, x8):
    """The composition with every sign positive."""
    def P(s, prefix=""):
        return INV._poly(s.replace("-", "+"), x8, prefix=prefix)
    if name == "polynomial":
        return torch.cat([x8[0]] + [P(s) for s in INV._DEG2 + INV._DEG3 + INV._DEG4], dim=-1)
    return torch.cat([x8[0] ** 3] + [P(s, "0") for s in INV._DEG2] + [P(s) for s in INV._DEG3], dim=-1)


def oracle_bwd(name, xp, g, c):
    """float64 on the CPU: (dx, S) packed like xp - autograd of the composition, and of its all-positive twin at |x|, |g|."""
    x = xp.detach().cpu().double().requires_grad_()
    g = g.detach().cpu().double()
    (dx,) = torch.autograd.grad(stock(name, x, c), x, g)
    a = x.detach().abs().requires_grad_()
    (S,) = torch.autograd.grad(_abs_forward(name, _x8(a, c)), a, g.abs())
    return dx, S


def bound_bwd(name, S, c):
    T = torch.tensor([TERMS[name][j] for j in SLOT], dtype=torch.float64).repeat_interleave(c)
    return (T + 8) * EPS * S


class Guarded:
    """n elements of dtype inside a buffer with 64-element sentinel bands on both sides."""
    BAND = 64

    def __init__(self, n, dtype):
        self.sent = -12345.0
        self.buf = torch.full((n + 2 * self.BAND,), self.sent, dtype=dtype, device=DEV)
        self.t = self.buf[self.BAND:self.BAND + n]

    def ok(self):
        return bool((self.buf[:self.BAND] == self.sent).all() and (self.buf[-self.BAND:] == self.sent).all())


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _x_view(xp, c, layout, pad_rows=3):
    """Device copy of packed rows xp [M, 8c] as a packed or row-strided view (ld = 8c + 8), NaN rows behind row M - 1 and NaN
    in the pad columns."""
    M = xp.shape[0]
    ld = 8 * c + (8 if layout == "strided" else 0)
    buf = torch.full((M + pad_rows, ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:M, :8 * c] = xp.to(DEV)
    return buf[:M, :8 * c], buf


def run_fwd(name, xp, c, out_dt, layout):
    """octic_poly_invariant_fwd through the C ABI on a guarded output."""
    M = xp.shape[0]
    xv_t, keep = _x_view(xp, c, layout)
    xv = ops._orbit_view(xv_t, c)
    out = Guarded(M * NP[name] * c, out_dt)
    _lib.check(lib().octic_poly_invariant_fwd(ctypes.byref(xv), _p(out.t), M, c, ops.POLY_MAPS[name][0], ops.dt_code(out_dt), _stream()))
    torch.cuda.synchronize()
    assert out.ok(), "out: guard band overwritten"
    assert torch.isnan(keep[M:]).all()
    return out.t.view(M, NP[name] * c).clone()


def run_bwd(name, g, xp, c, layout):
    """octic_poly_invariant_bwd through the C ABI: x packed or row-strided, dx in a guarded buffer."""
    M = xp.shape[0]
    xv_t, keep = _x_view(xp, c, layout)
    xv = ops._orbit_view(xv_t, c)
    dx = Guarded(M * 8 * c, torch.float32)
    dv = ops.pview(dx.t.view(M, 8 * c), c)
    gd = g.to(DEV).contiguous()
    _lib.check(lib().octic_poly_invariant_bwd(_p(gd), ops.dt_code(gd.dtype), ctypes.byref(xv), ctypes.byref(dv), M, c,
                                              ops.POLY_MAPS[name][0], _stream()))
    torch.cuda.synchronize()
    assert dx.ok(), "dx: guard band overwritten"
    return dx.t.view(M, 8 * c).clone()


def same_bits(a, b):
    """Equal bit patterns wherever neither is NaN, and equal NaN masks."""
    assert a.dtype == b.dtype and a.shape == b.shape
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    it = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.contiguous().view(it)[~na], b.contiguous().view(it)[~nb])


@functools.lru_cache(maxsize=None)
def normal_x(M, c):
    """Seeded normal rows [M, 8c] (CPU) with rows of zeros, denormals, +inf, -inf and NaN entries planted at rows 1 .. 5."""
    gen = torch.Generator().manual_seed(100 * M + c)
    x = torch.randn(M, 8 * c, generator=gen)
    if M > 1:
        x[1] = 0.0
    if M > 2:
        x[2] *= 1e-39                         # denormal float32 values
        assert ((x[2] != 0) & (x[2].abs() < 2.0 ** -126)).any()
    if M > 5:
        x[3, ::3] = float("inf")
        x[4, ::5] = float("-inf")
        x[5, ::7] = float("nan")
    return x


@functools.lru_cache(maxsize=None)
def stock_fwd(name, M, c):
    """The stock arm's f32 output on the GPU for normal_x(M, c): computed once, shared, never modified."""
    return stock(name, normal_x(M, c).to(DEV), c)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_forward_bitwise(name, dtn, c, M):
    dt = DT[dtn]
    xp = normal_x(M, c)
    want32 = stock_fwd(name, M, c)
    assert want32.dtype == torch.float32 and want32.shape == (M, NP[name] * c)
    want = want32 if dt == torch.float32 else want32.to(torch.bfloat16)
    if M > 5:
        assert torch.isnan(want[5]).any() and torch.isinf(want[3]).any() and torch.isfinite(want[6:]).all()
    for layout in ("packed", "strided"):
        assert same_bits(run_fwd(name, xp, c, dt, layout), want), layout
        xv_t, _ = _x_view(xp, c, layout)
        assert M == 1 or xv_t.is_contiguous() == (layout == "packed")
        assert same_bits(ops.poly_invariant_fwd(xv_t, c, name, dt), want), ("ops", layout)
    # the non-NaN part is plain equality too, as the issue states it
    fin = ~torch.isnan(want).any(dim=1)
    assert torch.equal(run_fwd(name, xp, c, dt, "packed")[fin], want[fin])


# ------------------------------------------------------------------------------------------ backward
@functools.lru_cache(maxsize=None)
def integer_case(name, M, c):
    """Small-integer x, g (CPU, f32) with every component and every cotangent plane non-zero somewhere and every generator
    non-zero somewhere, and the float64 autograd of the composition."""
    P = NP[name]
    for attempt in range(200):
        gen = torch.Generator().manual_seed(7919 * attempt + 100 * M + c)
        x = torch.randint(-3, 4, (M, 8 * c), generator=gen).float()
        g = torch.randint(-4, 5, (M, P * c), generator=gen).float()
        y = stock(name, x.double(), c)
        if (x.view(M, 8, c) != 0).any(2).any(0).all() and (g.view(M, P, c) != 0).any(2).any(0).all() \
                and (y.view(M, P, c) != 0).any(2).any(0).all():
            dx, _ = oracle_bwd(name, x, g, c)
            assert dx.abs().max() < 2 ** 24
            return x, g, dx
    raise AssertionError("no draw with every generator non-zero")


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_backward_exact_on_small_integers(name, dtn, c, M):
    x, g, dx64 = integer_case(name, M, c)
    gq = g.to(DT[dtn])
    assert torch.equal(gq.float(), g)
    for layout in ("packed", "strided"):
        dx = run_bwd(name, gq, x, c, layout)
        assert torch.equal(dx.cpu().double(), dx64), layout
    assert torch.equal(ops.poly_invariant_bwd(gq.to(DEV), x.to(DEV), c, name).cpu().double(), dx64)
    # forward on the same operands: exact as well (f32 output; every generator is an integer below 2^24)
    assert torch.equal(run_fwd(name, x, c, torch.float32, "packed").cpu().double(), stock(name, x.double(), c))


@functools.lru_cache(maxsize=None)
def random_case(name, dtn, M, c):
    gen = torch.Generator().manual_seed(31 * M + c + 1)
    x = torch.randn(M, 8 * c, generator=gen)
    g = torch.randn(M, NP[name] * c, generator=gen).to(DT[dtn])
    dx64, S = oracle_bwd(name, x, g, c)
    return x, g, dx64, bound_bwd(name, S, c)


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_backward_random_against_float64(name, dtn, c, M):
    x, g, dx64, bound = random_case(name, dtn, M, c)
    dx = run_bwd(name, g, x, c, "packed").cpu().double()
    err = (dx - dx64).abs()
    print(f"{name} {dtn} c={c} M={M}: max error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------ invariances
def _group_operands():
    M, c = 70, 24
    xp = torch.randn(M, 8 * c, generator=torch.Generator().manual_seed(9)).to(DEV)
    x8 = _x8(xp, c)
    moved = {g: _pack8([_ISO[g][1][i] * x8[_ISO[g][0][i]] for i in range(8)]).contiguous() for g in group_elements}
    assert all(g == "e" or not torch.equal(moved[g], xp) for g in group_elements)
    return M, c, xp, moved


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_out_is_bitwise_invariant_under_the_group(name, dtn):
    """out is bitwise unchanged under each of the eight group elements.  This rests on the order of the digits in the monomial
    tables (d8_invariantization._DEG3 / _DEG4): r, rrr, mr and mrrr exchange x4 <-> x5 and x6 <-> x7, and a left-to-right
    float32 product depends on the order of its factors, so the tables list every two-term generator's second monomial as the
    digit-by-digit image of its first and let one-term generators multiply an exchanged pair first.  With the digit order of
    the reference's source ("367", "1245", "16667-16777", ...) 5540 of these 53760 polynomial f32 outputs differed under each
    swapping element, by up to 256 ulp."""
    M, c, xp, moved = _group_operands()
    base = ops.poly_invariant_fwd(xp, c, name, DT[dtn])
    for g in group_elements:
        got = ops.poly_invariant_fwd(moved[g], c, name, DT[dtn])
        assert same_bits(got, base) and torch.equal(got, base), g
        if dtn == "f32":
            assert torch.equal(got, stock(name, moved[g], c)), g     # and the stock arm has the same property


@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_rows_do_not_depend_on_batch_mates_position_or_repetition(name, dtn):
    M, c = 150, 40
    torch.manual_seed(3)
    x = torch.randn(M, 8 * c, device=DEV)
    g = torch.randn(M, NP[name] * c, device=DEV).to(DT[dtn])

    def run(xx, gg):
        return ops.poly_invariant_fwd(xx, c, name, DT[dtn]), ops.poly_invariant_bwd(gg, xx, c, name)

    a, b = run(x, g), run(x, g)
    assert all(torch.equal(p, q) for p, q in zip(a, b)), "two calls differ"
    perm = torch.randperm(M, device=DEV)[:77]
    s = run(x[perm].contiguous(), g[perm].contiguous())
    assert torch.equal(s[0], a[0][perm]) and torch.equal(s[1], a[1][perm])
    one = run(x[41:42].contiguous(), g[41:42].contiguous())
    assert torch.equal(one[0], a[0][41:42]) and torch.equal(one[1], a[1][41:42])
    # a NaN row (in x and in g) leaves every other row's dx bit-identical
    xn, gn = x.clone(), g.clone()
    xn[17], gn[17] = float("nan"), float("nan")
    dn = ops.poly_invariant_bwd(gn, xn, c, name)
    keep = torch.arange(M, device=DEV) != 17
    assert torch.isnan(dn[17]).all() and torch.equal(dn[keep], a[1][keep])


# ------------------------------------------------------------------------------------------ 64-bit offsets
def test_offsets_past_2_to_31_elements():
    """Polynomial map, c = 160, M = 420 000: out and g hold 2.15e9 elements (bf16, 4.3 GB each), x and dx 5.4e8.  The last rows
    lie behind element 2^31 of out; forward and dx are compared on the first and last 64 rows with a 64-row call each (rows do
    not depend on position, tested above) - the launcher has no grid cap, this is its one large-size path."""
    name, c, M = "polynomial", 160, 420_000
    assert M * 32 * c > 2 ** 31
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randn(M, 8 * c, device=DEV, generator=gen)
    out = ops.poly_invariant_fwd(x, c, name, torch.bfloat16)
    for sl in (slice(0, 64), slice(M - 64, M)):
        assert torch.equal(out[sl], stock(name, x[sl].contiguous(), c).to(torch.bfloat16))
    g = out                                      # any finite bf16 cotangent will do: reuse the 4.3 GB
    dx = ops.poly_invariant_bwd(g, x, c, name)
    for sl in (slice(0, 64), slice(M - 64, M)):
        assert torch.equal(dx[sl], ops.poly_invariant_bwd(g[sl].contiguous(), x[sl].contiguous(), c, name))
    mid = slice(M // 2, M // 2 + 64)
    assert torch.equal(dx[mid], ops.poly_invariant_bwd(g[mid].contiguous(), x[mid].contiguous(), c, name))


# ------------------------------------------------------------------------------------------ memory
@pytest.mark.parametrize("dtn", ["f32", "bf16"])
@pytest.mark.parametrize("name", sorted(MODS))
def test_peak_memory_and_the_one_saved_tensor(name, dtn):
    """Over forward + backward the peak above what is resident (x and the cotangent handed to backward) is at most
    bytes(out) + bytes(g) + bytes(dx) plus the allocator's rounding: the caching allocator rounds every block to a multiple
    of 512 bytes, three blocks.  The one saved tensor is the contiguous f32 input itself."""
    dt, M, c = DT[dtn], 2056, 40
    P, es = NP[name], DT[dtn].itemsize
    x = torch.randn(8, M // 8, 8 * c, device=DEV).requires_grad_()
    gout = torch.randn(8, M // 8, P * c, device=DEV).to(dt)
    mod = MODS[name](8 * c)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dt == torch.bfloat16):
        y = mod(OF.Octic(x, c), _out_dtype=dt)
    assert y.dtype == dt and y.shape == gout.shape
    saved = y.grad_fn.saved_tensors
    assert len(saved) == 1 and saved[0].dtype == torch.float32
    assert saved[0].untyped_storage().data_ptr() == x.untyped_storage().data_ptr() and saved[0].data_ptr() == x.data_ptr()
    y.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    limit = y.numel() * es + gout.numel() * es + x.numel() * 4 + 3 * 512
    print(f"{name} {dtn}: peak {peak / 2 ** 20:.2f} MiB, limit {limit / 2 ** 20:.2f} MiB")
    assert peak <= limit
    assert x.grad is not None and x.grad.dtype == torch.float32 and x.grad.shape == x.shape


def test_module_takes_a_plain_5_tuple_and_refused_inputs_run_the_composition():
    c = 16
    torch.manual_seed(2)
    xp = torch.randn(3, 11, 8 * c, device=DEV)
    for name, cls in MODS.items():
        mod = cls(8 * c)
        want = stock(name, xp, c)
        got = mod(ops.split_packed(xp, c))                       # a reference-style 5-tuple: one torch.cat, then the kernel
        assert torch.equal(got, want) and got.shape == (3, 11, NP[name] * c)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert INV.poly_hip_ok(OF.Octic(xp, c))
            assert torch.equal(mod(OF.Octic(xp, c), _out_dtype=torch.bfloat16), want.to(torch.bfloat16))
        with torch.autocast("cuda", dtype=torch.float16):
            assert INV.poly_hip_ok(OF.Octic(xp, c))
        xb = xp.bfloat16()
        assert not INV.poly_hip_ok(OF.Octic(xb, c))
        assert torch.equal(mod(OF.Octic(xb, c)), stock(name, xb, c)) and mod(OF.Octic(xb, c)).dtype == torch.bfloat16
    with pytest.raises(ValueError):
        ops.poly_invariant_fwd(xp, c, "power_spectrum", torch.float32)
    with pytest.raises(TypeError):
        ops.poly_invariant_fwd(xp.bfloat16(), c, "polynomial", torch.float32)


# ------------------------------------------------------------------------------------------ models
def _inv_model(name, seed=0):
    from octic_vits_amd.model import OcticVisionTransformer
    torch.manual_seed(seed)
    return OcticVisionTransformer(img_size=32, patch_size=4, in_chans=3, num_classes=10, embed_dim=128, depth=2, num_heads=2,
                                  mlp_ratio=4.0, drop_path_rate=0.0, invariant=True, invariantization=name).cuda()


@pytest.mark.parametrize("name", sorted(MODS))
def test_model_logits_are_bitwise_equal_on_both_arms(name, monkeypatch):
    net = _inv_model(name)
    assert isinstance(net.invariantization, MODS[name])
    x = torch.randn(4, 3, 32, 32, device=DEV)
    outs = []
    for hip in (True, False):
        monkeypatch.setattr(INV, "POLY_HIP", hip)
        with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
            outs.append(net(x))
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name", sorted(MODS))
def test_model_trains_eager_and_captured_bitwise(name):
    from octic_vits_amd.train import Trainer, synthetic_batch
    ma, mb = _inv_model(name), _inv_model(name)
    ta, tb = Trainer(ma, lr=1e-3), Trainer(mb, lr=1e-3)
    batches = [synthetic_batch(8, 10, "cuda", seed=s, img_size=32) for s in range(3)]
    gs = tb.capture(*batches[0], warmup=2)
    for _ in range(2):
        ta.step(*batches[0])
    la = [float(ta.step(x, y).detach()) for x, y in batches[1:]]
    lb = [float(gs.replay(x, y)) for x, y in batches[1:]]
    assert la == lb and all(v == v for v in la)
    for (n, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert torch.equal(pa, pb), n


@pytest.mark.parametrize("name", sorted(MODS))
def test_model_first_backward_against_float64(name):
    """One Trainer.step of the 2-block model (bf16 autocast).  Hooks take the block output the hand-off receives, the map's
    output and the cotangents that arrive at each; the float64 replica of the map runs on that block output with that cotangent
    (bf16, as it arrived), and the cotangent at the block output stays within (T_i + 8) 2^-24 S_i of it."""
    from octic_vits_amd.train import Trainer, synthetic_batch
    net = _inv_model(name, seed=3)
    cap = {}

    def pre(mod, args, kwargs):
        xs = args[0]
        assert isinstance(xs, OF.Octic)
        cap["x"], cap["c"], cap["out_dtype"] = xs.packed.detach().clone(), xs.c, kwargs.get("_out_dtype")
        xs.packed.register_hook(lambda g: cap.__setitem__("dx", g.detach().clone()))

    def post(mod, args, kwargs, out):
        cap["y"] = out.detach().clone()
        out.register_hook(lambda g: cap.__setitem__("gy", g.detach().clone()))

    inv = net.invariantization
    hs = [inv.register_forward_pre_hook(pre, with_kwargs=True), inv.register_forward_hook(post, with_kwargs=True)]
    loss = float(Trainer(net, lr=1e-3).step(*synthetic_batch(8, 10, "cuda", seed=1, img_size=32)))
    torch.cuda.synchronize()
    for h in hs:
        h.remove()
    assert loss == loss
    c, x, y, gy, dx = cap["c"], cap["x"], cap["y"], cap["gy"], cap["dx"]
    assert c == 16 and x.dtype == torch.float32 and cap["out_dtype"] == torch.bfloat16
    assert y.dtype == torch.bfloat16 and gy.dtype == torch.bfloat16 and dx.dtype == torch.float32 and dx.shape == x.shape
    M = x.numel() // (8 * c)
    assert torch.equal(y.view(M, -1), stock(name, x.view(M, 8 * c), c).to(torch.bfloat16))      # the step ran the stock bits
    dx64, S = oracle_bwd(name, x.view(M, 8 * c), gy.view(M, -1), c)
    bound = bound_bwd(name, S, c)
    err = (dx.view(M, 8 * c).cpu().double() - dx64).abs()
    print(f"model {name}: dx max error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert (err <= bound).all()
