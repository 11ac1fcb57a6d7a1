"""Invariant maps (reference: octic_vits/d8_invariantization.py).

PowerSpectrumInvariant — the models' default (model.py:89-91) — is a HIP kernel (fwd + bwd), and so are the two orbit-based
maps with learned parameters, MaxFilteringInvariant and CanonizationInvariant (csrc/orbit_invariant.hip: all eight products
of an orbit from 12 partial dots, nothing eightfold in memory); `orbit_hip_ok` is their routing rule, and what it refuses
runs the reference's composition from the group-action tables of d8_utils.  The polynomial maps (PolynomialInvariant,
ThirdOrderInvariant) are defined by a compact monomial table ("356+347" = x3*x5*x6 + x3*x4*x7); on float32 GPU tensors they
are one fused kernel forward and one backward (csrc/poly_invariant.hip, `poly_hip_ok` is the routing rule) that evaluate the
same expression trees in float32 without fma, so the result equals the table-driven torch composition bit for bit; what the
rule refuses - CPU tensors, bf16 / fp16 tensors, torch.compile tracing - runs that composition.  The digits of the tables are
ordered so that both arms are invariant under the eight group elements bit for bit.  LinearInvariant is one `abs`.
"""
import inspect
import os
import re

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import functional as OF
from .d8_utils import _ISO, convert_5tuple_to_8tuple, group_elements
from .functional import as_packed


ORBIT_HIP = os.environ.get("OCTIC_ORBIT_HIP", "1") != "0"     # MaxFiltering / Canonization on the HIP kernels where they can run


def orbit_hip_ok(xtuple, *params) -> bool:
    """The one routing rule of the orbit kernels: GPU tensors, a float32 / bfloat16 input whose compute dtype is one of the
    two, c a multiple of 8, not under torch.compile tracing, and the switch ORBIT_HIP on."""
    if not ORBIT_HIP or torch.compiler.is_compiling():
        return False
    ts = [xtuple.packed] if isinstance(xtuple, OF.Octic) else list(xtuple)
    if len(ts) not in (1, 5) or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts + list(params)):
        return False
    if any(t.dtype not in (torch.float32, torch.bfloat16) for t in ts) or any(p.dtype != torch.float32 for p in params):
        return False
    if torch.is_autocast_enabled("cuda"):
        adt = torch.get_autocast_dtype("cuda")
        # fp16 autocast computes the octic half in float32 and takes float32 inputs only (functional.compute_dtype)
        if adt not in (torch.bfloat16, torch.float16) or (adt == torch.float16 and any(t.dtype != torch.float32 for t in ts)):
            return False
    c = xtuple.c if isinstance(xtuple, OF.Octic) else ts[0].shape[-1]
    return c > 0 and c % 8 == 0 and ts[0].numel() > 0


POLY_HIP = os.environ.get("OCTIC_POLY_HIP", "1") != "0"       # Polynomial / ThirdOrder on the HIP kernels where they can run


def poly_hip_ok(xtuple) -> bool:
    """The one routing rule of the polynomial kernels: the switch POLY_HIP on, not under torch.compile tracing (Inductor fuses
    the composition itself), non-empty float32 GPU tensors and c a positive multiple of 8.  Any autocast state passes: the
    arithmetic is float32 either way.  bf16 / fp16 tensors stay on the composition, which rounds per operation."""
    if not POLY_HIP or torch.compiler.is_compiling():
        return False
    ts = [xtuple.packed] if isinstance(xtuple, OF.Octic) else list(xtuple)
    if len(ts) not in (1, 5) or not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    c = xtuple.c if isinstance(xtuple, OF.Octic) else ts[0].shape[-1]
    return c > 0 and c % 8 == 0 and all(t.numel() > 0 for t in ts)


class Invariant(nn.Module):
    """Base class for invariants (d8_invariantization.py:12-18)."""

    def __init__(self, dim: int):
        super().__init__()
        self.output_dim = dim


def invariant_head_factory(invariant: Invariant, C: int, num_classes: int, norm=False):
    """d8_invariantization.py:20-28."""
    return nn.Sequential(
        nn.LayerNorm(invariant.output_dim, eps=1e-6) if norm else nn.Identity(),
        nn.Linear(invariant.output_dim, C), nn.GELU(),
        nn.Linear(C, num_classes) if num_classes > 0 else nn.Identity())


class NonInvariant(Invariant):  # :29-42
    def __init__(self, C: int):
        super().__init__(C)

    def forward(self, xtuple):
        return torch.cat([x.abs() for x in convert_5tuple_to_8tuple(xtuple)], dim=-1)


class LinearInvariant(Invariant):  # :43-48
    def __init__(self, C: int):
        super().__init__(C // 8)

    def forward(self, xtuple, _out_dtype=None):
        return torch.abs(xtuple[0])


class PowerSpectrumInvariant(Invariant):  # :49-64 -> octic_power_spectrum_fwd/bwd
    def __init__(self, C: int):
        super().__init__(6 * C // 8)

    def forward(self, xtuple, _out_dtype=None):
        xp, c = as_packed(xtuple)
        return OF.PowerSpectrumFn.apply(xp, c, _out_dtype or xp.dtype)


# monomial tables: digits are 8-tuple indices, repeated digits are powers.  A monomial is evaluated as the left-to-right product
# of its digits, so the ORDER of the digits is part of the float32 result.  It is chosen so that every generator is invariant
# bit for bit, not only up to rounding: the four group elements that exchange x4 <-> x5 and x6 <-> x7 map a two-term generator's
# first string onto its second digit by digit ("14456" -> "15547"), and a one-term generator that holds such a pair multiplies
# the pair first ("673": x6 * x7 == x7 * x6).  The other four elements only flip signs.
_DEG2 = ["66+77", "46+57", "44+55", "33", "22", "11"]
_DEG3 = ["673", "356+347", "453", "266-277", "246-257", "244-255", "156-147", "123"]
_DEG4 = ["6666+7777", "4666+5777", "4466+5577", "4446+5557", "4444+5555", "2356-2347", "1366-1377", "1346-1357",
         "1344-1355", "6712", "1256+1247", "4512", "16667-17776", "15666-14777", "14566-15477", "14456-15547",
         "14445-15554"]


def _poly(spec, x, prefix=""):
    out = None
    for sign, digits in re.findall(r"([+-]?)(\d+)", spec):
        term = None
        for d in prefix + digits:
            term = x[int(d)] if term is None else term * x[int(d)]
        out = (term if sign != "-" else -term) if out is None else (out + term if sign != "-" else out - term)
    return out


class PolynomialInvariant(Invariant):  # :66-112 -> octic_poly_invariant_fwd/bwd
    def __init__(self, C: int):
        super().__init__(32 * C // 8)

    def forward(self, xtuple, _out_dtype=None):
        if poly_hip_ok(xtuple):
            xp, c = as_packed(xtuple)
            return OF.PolyInvariantFn.apply(xp, c, "polynomial", _out_dtype or xp.dtype)
        x = convert_5tuple_to_8tuple(xtuple)
        return torch.cat([x[0]] + [_poly(s, x) for s in _DEG2 + _DEG3 + _DEG4], dim=-1)


class ThirdOrderInvariant(Invariant):  # :114-141 -> octic_poly_invariant_fwd/bwd
    def __init__(self, C: int):
        super().__init__(15 * C // 8)

    def forward(self, xtuple, _out_dtype=None):
        if poly_hip_ok(xtuple):
            xp, c = as_packed(xtuple)
            return OF.PolyInvariantFn.apply(xp, c, "third_order", _out_dtype or xp.dtype)
        x = convert_5tuple_to_8tuple(xtuple)
        return torch.cat([x[0] ** 3] + [_poly(s, x, prefix="0") for s in _DEG2] + [_poly(s, x) for s in _DEG3], dim=-1)


def _action_matrix(g):
    perm, sign = _ISO[g]
    m = torch.zeros(8, 8)
    for i in range(8):
        m[i, perm[i]] = sign[i]
    return m


def _orbit_matrices():
    return [_action_matrix(g) for g in group_elements]  # e, r, rr, rrr, m, mr, mrr, mrrr  (:186-199)


class MaxFilteringInvariant(Invariant):  # :142-210
    def __init__(self, input_channels: int, num_references=None, learnable_references: bool = True,
                 global_avg: bool = False):
        if num_references is None:
            num_references = input_channels * 2
        super().__init__(num_references)
        self.references = nn.Parameter(F.normalize(torch.randn(num_references, input_channels // 8, 8), dim=(1, 2)),
                                       requires_grad=learnable_references)
        self.rotation_action = nn.Parameter(_action_matrix("r"), requires_grad=False)
        self.reflection_action = nn.Parameter(_action_matrix("m"), requires_grad=False)
        self.global_avg = global_avg

    def expand_references_d8(self):
        mats = torch.stack(_orbit_matrices()).to(self.references)          # [8 g, 8, 8]
        return torch.einsum("gij,dcj->gdic", mats, self.references).flatten(start_dim=-2)

    def forward(self, xtuple, _out_dtype=None):
        if orbit_hip_ok(xtuple, self.references):
            xp, c = as_packed(xtuple)
            if c != self.references.shape[1]:
                raise ValueError(f"MaxFilteringInvariant: input has c = {c}, the references have {self.references.shape[1]}")
            return OF.MaxFilterFn.apply(xp, self.references, c, _out_dtype or OF.compute_dtype(xp))
        x = torch.cat(convert_5tuple_to_8tuple(xtuple), dim=-1)
        refs = self.expand_references_d8()
        prod = torch.einsum("kdc,bc->bkd", refs, x) if self.global_avg else torch.einsum("kdc,bnc->bnkd", refs, x)
        return prod.max(dim=-2).values


class CanonizationInvariant(Invariant):  # :212-280
    def __init__(self, dim, learnable_reference=True, global_avg=False):
        super().__init__(dim)
        self.reference = nn.Parameter(F.normalize(torch.randn(dim), dim=0), requires_grad=learnable_reference)
        self.rotation_action = nn.Parameter(_action_matrix("r"), requires_grad=False)
        self.reflection_action = nn.Parameter(_action_matrix("m"), requires_grad=False)
        self.global_avg = global_avg

    def expand_x_d8(self, x):
        mats = torch.stack(_orbit_matrices()).to(x)
        return torch.einsum("gij,...cj->...gic", mats, x).flatten(start_dim=-2)

    def forward(self, xtuple, _out_dtype=None):
        if orbit_hip_ok(xtuple, self.reference):
            xp, c = as_packed(xtuple)
            if 8 * c != self.reference.numel():
                raise ValueError(f"CanonizationInvariant: input has {8 * c} channels, the reference has {self.reference.numel()}")
            return OF.CanonizeFn.apply(xp, self.reference, c, _out_dtype or OF.compute_dtype(xp))
        x = torch.stack(convert_5tuple_to_8tuple(xtuple), dim=-1)
        if self.global_avg:
            x = x.unsqueeze(1)
        orbit = self.expand_x_d8(x)
        best = torch.einsum("c,bnkc->bnk", self.reference, orbit).argmax(dim=-1, keepdim=True)
        out = torch.gather(orbit, 2, best.unsqueeze(-1).expand(-1, -1, -1, orbit.shape[-1])).squeeze(-2)
        return out.squeeze(1) if self.global_avg else out


INVARIANTIZATIONS = {"linear": LinearInvariant, "power_spectrum": PowerSpectrumInvariant, "polynomial": PolynomialInvariant,
                     "third_order": ThirdOrderInvariant, "max_filtering": MaxFilteringInvariant,
                     "canonization": CanonizationInvariant}


def make_invariantization(spec, embed_dim: int) -> Invariant:
    """The invariant map of a model built with invariant=True: one of the names above, or a callable embed_dim -> Invariant
    whose forward takes the keyword `_out_dtype` (the models pass it; the stock maps take and ignore it)."""
    if callable(spec):
        inv = spec(embed_dim)
        if not isinstance(inv, Invariant):
            raise TypeError(f"invariantization callable must return an Invariant, got {type(inv).__name__}")
        params = inspect.signature(inv.forward).parameters
        if "_out_dtype" not in params and not any(p.kind == p.VAR_KEYWORD for p in params.values()):
            raise TypeError(f"{type(inv).__name__}.forward must take the keyword _out_dtype (the models pass it)")
        return inv
    if spec not in INVARIANTIZATIONS:
        raise ValueError(f"invariantization must be one of {sorted(INVARIANTIZATIONS)} or a callable, got {spec!r}")
    return INVARIANTIZATIONS[spec](embed_dim)
