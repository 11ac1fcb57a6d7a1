"""CPU-only checks of the polynomial invariants (PolynomialInvariant / ThirdOrderInvariant) on the engine: the two symbols, the
launchers' refusals, the routing predicate, and the CPU composition against the reference's goldens.  No kernel is launched."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import cases
from octic_vits_amd import _lib
from octic_vits_amd import d8_invariantization as INV
from octic_vits_amd.d8_utils import convert_8tuple_to_5tuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("octic_poly_invariant_fwd", "octic_poly_invariant_bwd")
POLY, THIRD = 0, 1


def test_symbols_are_declared_exported_documented_and_bound():
    declared = _lib.header_symbols()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = _lib.lib()
    for s in SYMBOLS:
        assert s in declared and s in _lib._PROTOS and s in text and hasattr(L, s), s
    assert "octic_vits/d8_invariantization.py:66-141" in text
    assert L.octic_abi_version() == _lib.ABI_VERSION == 20
    from octic_vits_amd import build, functional as OF, ops
    assert "poly_invariant.hip" in build.SOURCES
    assert callable(ops.poly_invariant_fwd) and callable(ops.poly_invariant_bwd)
    assert issubclass(OF.PolyInvariantFn, torch.autograd.Function)
    assert ops.POLY_MAPS == {"polynomial": (POLY, 32), "third_order": (THIRD, 15)}


def test_launchers_refuse_bad_arguments_before_launching():
    L = _lib.lib()
    v = _lib.OcticView()
    for i in range(5):
        v.ptr[i], v.ld[i] = 4096 + 64 * i, 64
    p, off = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    bv = ctypes.byref(v)
    F32, BF16 = _lib.F32, _lib.BF16
    fwd, bwd = L.octic_poly_invariant_fwd, L.octic_poly_invariant_bwd
    # Every call carries a second, independent flaw that a later check refuses (a pointer 4 bytes off), so a lost check cannot
    # turn this into a launch on placeholder addresses.  Order of the checks: NULL, dtype, shape, the views, alignment.
    assert fwd(bv, off, 4, 12, POLY, F32, None) == -1                       # c % 8 (then: out off)
    assert fwd(bv, off, 0, 8, POLY, F32, None) == -1                        # M < 1
    assert fwd(bv, off, 4, 8, 2, BF16, None) == -1                          # unknown map
    assert fwd(bv, off, 4, 8, -1, BF16, None) == -1
    assert fwd(bv, off, 2 ** 31, 8, THIRD, F32, None) == -1                 # offsets out of range: M c / 4 >= 2^31
    assert fwd(bv, off, 2 ** 62, 8, THIRD, F32, None) == -1
    assert fwd(bv, off, 4, 8, POLY, 2, None) == -3                          # dtype (then: out off)
    assert fwd(bv, None, 4, 12, POLY, F32, None) == -4                      # NULL (then: c % 8)
    assert fwd(None, off, 4, 12, POLY, F32, None) == -4
    assert bwd(off, F32, bv, bv, 4, 12, POLY, None) == -1                   # c % 8 (then: g off)
    assert bwd(off, F32, bv, bv, 0, 8, POLY, None) == -1
    assert bwd(off, BF16, bv, bv, 4, 8, 7, None) == -1
    assert bwd(off, F32, bv, bv, 2 ** 31, 8, POLY, None) == -1
    assert bwd(off, 2, bv, bv, 4, 8, THIRD, None) == -3
    assert bwd(None, F32, bv, bv, 4, 12, POLY, None) == -4
    assert bwd(off, F32, None, bv, 4, 8, POLY, None) == -4
    assert bwd(off, F32, bv, None, 4, 8, POLY, None) == -4
    v.ptr[1] = 4096 + 4                                                     # two misalignments: a view pointer and out / g
    assert fwd(bv, off, 4, 8, POLY, F32, None) == -2
    assert bwd(off, F32, bv, bv, 4, 8, POLY, None) == -2
    v.ptr[1] = 4096 + 64
    v.ptr[3] = 0                                                            # a NULL inside the view
    assert fwd(bv, off, 4, 8, POLY, F32, None) == -4
    v.ptr[3] = 4096 + 192
    v.ld[2] = 4                                                             # stride below the row
    assert fwd(bv, off, 4, 8, POLY, F32, None) == -1
    assert bwd(off, F32, bv, bv, 4, 8, POLY, None) == -1
    v.ld[2], v.ld[4] = 64, 24                                               # E stride below 4c
    assert fwd(bv, off, 4, 8, THIRD, BF16, None) == -1
    v.ld[4] = 66                                                            # a row stride that is no multiple of 16 bytes
    assert fwd(bv, off, 4, 8, THIRD, BF16, None) == -2


def _x8(B, N, c, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, N, c, generator=g) for _ in range(8)]


def test_predicate_refusals(monkeypatch):
    cpu = convert_8tuple_to_5tuple(_x8(1, 3, 8, 2))
    assert INV.POLY_HIP is True                                            # default on
    assert not INV.poly_hip_ok(cpu)                                        # CPU tensors
    assert not INV.poly_hip_ok(tuple(t.to("meta") for t in cpu))           # meta tensors
    assert not INV.poly_hip_ok(tuple(t.bfloat16() for t in cpu))
    assert not INV.poly_hip_ok(tuple(t.half() for t in cpu))

    class Gpu(torch.Tensor):                                               # a CPU tensor that says it is on the GPU
        is_cuda = True

    def fake(ts):
        return tuple(t.as_subclass(Gpu) for t in ts)

    assert INV.poly_hip_ok(fake(cpu))                                      # everything else about `cpu` passes ...
    assert not INV.poly_hip_ok(fake(t.bfloat16() for t in cpu))            # ... so these refusals are the dtype's,
    assert not INV.poly_hip_ok(fake(t.half() for t in cpu))
    assert not INV.poly_hip_ok(fake(convert_8tuple_to_5tuple(_x8(1, 3, 12, 2))))    # c % 8,
    assert not INV.poly_hip_ok(fake(convert_8tuple_to_5tuple(_x8(0, 3, 8, 2))))     # empty tensors,
    monkeypatch.setattr(INV, "POLY_HIP", False)
    assert not INV.poly_hip_ok(fake(cpu))                                  # the switch,
    monkeypatch.setattr(INV, "POLY_HIP", True)
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    assert not INV.poly_hip_ok(fake(cpu))                                  # and compile tracing


@pytest.mark.parametrize("name", ["inv_polynomial", "inv_thirdorder"])
def test_cpu_composition_matches_the_reference_goldens(name):
    """The stock arm is what every refused call runs.  Tolerance: the house tolerance of the float32 goldens
    (tests/test_modules_gpu.py: 1e-4 of each tensor's scale) - the goldens come from the reference's hand-written products,
    whose multiplication order differs from the tables' (the tables order the digits for bitwise invariance)."""
    ns = types.SimpleNamespace(PolynomialInvariant=INV.PolynomialInvariant, ThirdOrderInvariant=INV.ThirdOrderInvariant)
    got = cases.run_module_case(ns, name)
    want = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    assert set(got) == set(want.files)
    for k in want.files:
        w, g = want[k].astype(np.float64), got[k].astype(np.float64)
        scale = max(1.0, float(np.abs(w).max()))
        assert np.allclose(g, w, rtol=1e-4, atol=1e-4 * scale), (name, k, float(np.abs(g - w).max()), scale)


# the polynomials of the reference (octic_vits/d8_invariantization.py:66-141) as the tables listed them before the digits were ordered
REFERENCE = {"deg2": ["66+77", "46+57", "44+55", "33", "22", "11"],
             "deg3": ["367", "356+347", "345", "266-277", "246-257", "244-255", "156-147", "123"],
             "deg4": ["6666+7777", "4666+5777", "4466+5577", "4446+5557", "4444+5555", "2356-2347", "1366-1377", "1346-1357",
                      "1344-1355", "1267", "1256+1247", "1245", "16667-16777", "15666-14777", "14566-14577", "14456-14557",
                      "14445-14555"]}


def _as_polynomial(spec):
    """A table string as (sign, sorted digits) per term: the polynomial, whatever the order of the multiplies."""
    import re
    return [(sign != "-", "".join(sorted(digits))) for sign, digits in re.findall(r"([+-]?)(\d+)", spec)]


def test_tables_are_the_reference_polynomials_with_reordered_digits():
    for ours, ref in ((INV._DEG2, REFERENCE["deg2"]), (INV._DEG3, REFERENCE["deg3"]), (INV._DEG4, REFERENCE["deg4"])):
        assert len(ours) == len(ref)
        for a, b in zip(ours, ref):
            assert _as_polynomial(a) == _as_polynomial(b), (a, b)
    # and the kernel file holds the same strings, digit for digit
    text = open(os.path.join(ROOT, "octic_vits_amd", "csrc", "poly_invariant.hip")).read()
    for spec in INV._DEG2 + INV._DEG3 + INV._DEG4:
        assert f'"{spec}"' in text, spec


@pytest.mark.parametrize("cls,P", [(INV.PolynomialInvariant, 32), (INV.ThirdOrderInvariant, 15)])
def test_composition_is_bitwise_invariant_and_has_the_plane_layout(cls, P):
    """float32 on the CPU: P planes of width c, and every generator is invariant under the eight group elements bit for bit
    (the property the GPU test asks of the kernels; it rests on the order of the digits in the tables)."""
    from octic_vits_amd.d8_utils import _ISO, group_elements
    c = 64
    xs = _x8(4, 50, c, 5)
    mod = cls(8 * c)
    y = mod(convert_8tuple_to_5tuple(xs))
    assert y.shape == (4, 50, P * c) and mod.output_dim == P * c and y.dtype == torch.float32
    for g in group_elements:
        perm, sign = _ISO[g]
        moved = [sign[i] * xs[perm[i]] for i in range(8)]
        assert torch.equal(mod(convert_8tuple_to_5tuple(moved)).view(torch.int32), y.view(torch.int32)), g
