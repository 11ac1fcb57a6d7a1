"""CPU-only checks of the orbit invariants (MaxFiltering / Canonization) on the engine: the symbols, the 12-pair structure the
kernels rest on, the routing predicate and the models' `invariantization` keyword.  No kernel is launched."""
import ctypes
import os

import pytest
import torch

from octic_vits_amd import _lib
from octic_vits_amd import d8_invariantization as INV
from octic_vits_amd.d8_utils import convert_8tuple_to_5tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octic_max_filter_prep", "octic_max_filter_fwd", "octic_max_filter_bwd_x", "octic_max_filter_bwd_ref",
           "octic_max_filter_bwd_ref_plan", "octic_max_filter_bwd_ref_workspace_bytes", "octic_canonize_fwd", "octic_canonize_bwd")
PAIRS = {(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (4, 5), (5, 4), (5, 5), (6, 6), (6, 7), (7, 6), (7, 7)}


def test_symbols_are_declared_exported_documented_and_bound():
    declared = _lib.header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in _lib._PROTOS and s in text and hasattr(L, s), s
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    from octic_vits_amd import functional as OF, ops
    for name in ("max_filter_prep", "max_filter_fwd", "max_filter_bwd_x", "max_filter_bwd_ref", "canonize_fwd", "canonize_bwd"):
        assert callable(getattr(ops, name))
    assert issubclass(OF.MaxFilterFn, torch.autograd.Function) and issubclass(OF.CanonizeFn, torch.autograd.Function)


def test_launchers_refuse_bad_arguments_before_launching():
    L = _lib.lib()
    v = _lib.OcticView()
    for i in range(5):
        v.ptr[i], v.ld[i] = 4096 + 64 * i, 64
    p, off = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    bv = ctypes.byref(v)
    # Every call carries a second, independent flaw that a later check refuses (a pointer 4 bytes off, or c = 12), so a lost
    # check cannot turn this into a launch on placeholder addresses.
    assert L.octic_max_filter_fwd(bv, off, p, p, 4, 4, 12, _lib.F32, _lib.F32, None) == -1      # c % 8 (then: planes off)
    assert L.octic_max_filter_fwd(bv, off, p, p, 0, 4, 8, _lib.F32, _lib.F32, None) == -1       # M < 1
    assert L.octic_max_filter_fwd(bv, off, p, p, 4, 0, 8, _lib.F32, _lib.F32, None) == -1       # R < 1
    assert L.octic_max_filter_fwd(bv, p, p, p, 4, 4, 12, 2, _lib.F32, None) == -3               # dtype (then: c % 8)
    assert L.octic_max_filter_fwd(bv, None, p, p, 4, 4, 12, _lib.F32, _lib.F32, None) == -4     # NULL (then: c % 8)
    assert L.octic_max_filter_bwd_x(p, p, off, bv, 4, 2 ** 40, 8, _lib.F32, None) == -1          # offsets past 2^31
    assert L.octic_max_filter_bwd_ref(off, p, bv, p, p, 0, 4, 2 ** 40, 8, _lib.F32, None) == -1
    assert L.octic_max_filter_prep(p, off, 4, 12, _lib.BF16, None) == -1
    assert L.octic_canonize_bwd(p, 2, p, bv, 4, 12, _lib.F32, None) == -3
    v.ptr[1] = 4096 + 4                                                                          # a view pointer off as well
    assert L.octic_max_filter_fwd(bv, off, p, p, 4, 4, 8, _lib.F32, _lib.F32, None) == -2       # two misalignments
    assert L.octic_canonize_fwd(bv, p, p, p, 4, 12, _lib.F32, _lib.F32, None) == -1             # c % 8 (then: the view)
    v.ptr[1] = 4096 + 64
    v.ld[2] = 4                                                                                  # stride below the row
    assert L.octic_max_filter_fwd(bv, off, p, p, 4, 4, 8, _lib.F32, _lib.F32, None) == -1       # (then: planes off)
    # the slab plan is a function of the shape alone; slabs of at least 256 rows, at most 8
    out = (ctypes.c_int * 4)()
    assert L.octic_max_filter_bwd_ref_plan(257, 24, 8, out) == 0 and out[0] == 2 and out[1] % 32 == 0 and out[0] * out[1] >= 257
    assert L.octic_max_filter_bwd_ref_plan(256, 24, 8, out) == 0 and out[0] == 1
    assert L.octic_max_filter_bwd_ref_plan(16448, 2560, 160, out) == 0 and 1 <= out[0] <= 8
    assert L.octic_max_filter_bwd_ref_workspace_bytes(257, 24, 8) == 2 * 24 * 64 * 4


def test_action_matrices_touch_exactly_the_12_pairs():
    mats = INV._orbit_matrices()
    touched = {(i, j) for m in mats for i in range(8) for j in range(8) if m[i, j] != 0}
    assert touched == PAIRS
    for m in mats:                                               # signed permutations
        assert (m.abs().sum(0) == 1).all() and (m.abs().sum(1) == 1).all() and set(m.unique().tolist()) <= {-1., 0., 1.}


def _x8(B, N, c, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, c, generator=g, dtype=torch.float64) for _ in range(8)]


def test_partial_formula_equals_the_composition_in_float64():
    torch.manual_seed(0)
    c, R = 8, 24
    mats = torch.stack(INV._orbit_matrices()).double()
    xs = _x8(2, 5, c, 1)
    # MaxFiltering: products[t, g, d] = sum over the 12 pairs of A_g[i, j] P_ij[t, d],  P_ij = x_i . ref[:, :, j]
    mod = INV.MaxFilteringInvariant(8 * c, num_references=R).double()
    want = mod(convert_8tuple_to_5tuple(xs))
    ref = mod.references.detach()
    prod = 0
    for i, j in sorted(PAIRS):
        P = torch.einsum("bnc,dc->bnd", xs[i], ref[:, :, j])
        prod = prod + mats[:, i, j].view(1, 1, 8, 1) * P.unsqueeze(2)
    assert torch.allclose(prod.max(dim=2).values, want, rtol=0, atol=1e-12)
    # Canonization: dot_g = sum over the pairs of A_g[i, j] reference_i . x_j, out = A_g x for the argmax
    can = INV.CanonizationInvariant(8 * c).double()
    want = can(convert_8tuple_to_5tuple(xs))
    rv = can.reference.detach().view(8, c)
    dots = 0
    for i, j in sorted(PAIRS):
        dots = dots + mats[:, i, j].view(1, 1, 8) * torch.einsum("bnc,c->bn", xs[j], rv[i]).unsqueeze(-1)
    best = dots.argmax(-1)
    x8 = torch.stack(xs, dim=-2)                                  # [B, N, 8, c]
    got = torch.einsum("bnij,bnjc->bnic", mats[best], x8).flatten(-2)
    assert torch.equal(got, want)


def test_predicate_refusals(monkeypatch):
    c = 8
    cpu = convert_8tuple_to_5tuple([t.float() for t in _x8(1, 3, c, 2)])
    ref = torch.zeros(4, c, 8)
    assert not INV.orbit_hip_ok(cpu, ref)                                     # CPU tensors
    assert not INV.orbit_hip_ok(tuple(t.half() for t in cpu), ref)            # fp16 tensors
    meta = tuple(t.to("meta") for t in cpu)
    assert not INV.orbit_hip_ok(meta, ref.to("meta"))                         # not a GPU
    monkeypatch.setattr(INV, "ORBIT_HIP", False)
    assert not INV.orbit_hip_ok(cpu, ref)
    monkeypatch.setattr(INV, "ORBIT_HIP", True)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert not INV.orbit_hip_ok(cpu, ref)


def _tiny(cls, **kw):
    from octic_vits_amd.d8_layers import Layer_scale_init_BlockD8
    from octic_vits_amd.vit import Layer_scale_init_Block
    if cls == "deit":
        from octic_vits_amd.model import OcticVisionTransformer
        return OcticVisionTransformer(img_size=28, patch_size=14, num_classes=5, embed_dim=64, depth=2, num_heads=2,
                                      qkv_bias=True, octic_block_layers=Layer_scale_init_BlockD8,
                                      standard_block_layers=Layer_scale_init_Block, invariant=True, **kw)
    from octic_vits_amd.dinov2_models import OcticDinoVisionTransformer
    return OcticDinoVisionTransformer(img_size=28, patch_size=14, embed_dim=64, depth=2, num_heads=2, invariant=True, **kw)


@pytest.mark.parametrize("cls", ["deit", "dinov2"])
def test_default_model_keeps_its_modules_and_keys(cls):
    net = _tiny(cls)
    assert type(net.invariantization) is INV.PowerSpectrumInvariant
    assert net.invariant_proj.in_features == 6 * 64 // 8
    inv_keys = sorted(k for k in net.state_dict() if k.startswith("invariant"))
    assert inv_keys == ["invariant_proj.bias", "invariant_proj.weight"]
    assert sorted(net.state_dict()) == sorted(_tiny(cls, invariantization="power_spectrum").state_dict())


@pytest.mark.parametrize("name", sorted(INV.INVARIANTIZATIONS))
@pytest.mark.parametrize("cls", ["deit", "dinov2"])
def test_every_map_builds_and_trains_on_the_stock_arm(cls, name):
    torch.manual_seed(0)
    net = _tiny(cls, invariantization=name)
    assert type(net.invariantization) is INV.INVARIANTIZATIONS[name]
    assert net.invariant_proj.in_features == net.invariantization.output_dim
    if name == "power_spectrum":
        return                                                   # its forward is the HIP kernel: no CPU arm (GPU tests cover it)
    # the engine's patch embedding and blocks have no CPU arm, so the CPU run is the models' hand-off on a 5-tuple: the call
    # the three call sites make (the map with _out_dtype, then invariant_proj), forward and backward
    xs = convert_8tuple_to_5tuple([t.float().requires_grad_() for t in _x8(2, 5, 8, 3)])
    y = net.invariant_proj(net.invariantization(xs, _out_dtype=torch.float32))
    assert y.shape == (2, 5, 64) and torch.isfinite(y).all()
    y.square().mean().backward()
    assert net.invariant_proj.weight.grad is not None and torch.isfinite(net.invariant_proj.weight.grad).all()
    if name == "max_filtering":
        assert net.invariantization.references.grad is not None


def test_keyword_takes_a_callable_and_refuses_unknown_names():
    net = _tiny("deit", invariantization=lambda d: INV.MaxFilteringInvariant(d, num_references=24, learnable_references=False))
    assert net.invariant_proj.in_features == 24 and not net.invariantization.references.requires_grad
    with pytest.raises(ValueError):
        _tiny("deit", invariantization="no_such_map")
    with pytest.raises(TypeError):
        _tiny("deit", invariantization=lambda d: torch.nn.Identity())

    class NoKeyword(INV.Invariant):
        def forward(self, xtuple):
            return xtuple[0]
    with pytest.raises(TypeError, match="_out_dtype"):
        _tiny("deit", invariantization=lambda d: NoKeyword(d // 8))
