"""The resident attention kernels (csrc/attention.hip, csrc/attn80*.hip: K and V, or Q and dO, of one head in LDS at once)
at every head_dim the entry points accept and at the token counts where the launch code changes kernel, against float64
softmax attention on the same bf16-rounded inputs, with NaN guard rows behind every input and sentinel rows behind every
output.

Which kernel a (T, hd) runs is written out in tests/test_attn_plan_host.py (FWD / BWD and the knob rows: the table that
octic_attn_plan, the library's one routing function, is held to on the host); the ids of the sweep below name it, and
test_sweep_reaches_every_kernel_a_resident_shape_can_reach holds the sweep to the table and the table to the library.
Names used in the ids: persist = attn_fwd_persist_kernel; attn80 = csrc/attn80.hip; fwd512 / fwd640w<waves> =
attn_fwd_kernel<KS, DT, 512 | 640>, one wave per query tile; attn80_bwd = the single-pass backward; pair512 / pair640 =
attn_bwd_dq_kernel + attn_bwd_dkv_kernel; "tile9": eight waves share the ninth tile (store_partial / combine_store) with
T - 256 = 1 .. 32 real rows; stream = csrc/attn_stream.hip, where the head's images exceed 160 KiB.

Bounds (the project's, test_attention_gpu.py): o max-abs <= 2e-2 max(1, max|ref|); lse <= 2e-3; gradients max-abs <= 3e-2
max(1, max|ref|); every tensor ||got - ref|| < 1.2e-2 max(||ref||, 1e-3) (the absolute floor is for dq / dk at T = 1, which
are zero in exact arithmetic).  _rounding_model is float64 attention with only the kernels' roundings (P and dS to bf16,
outputs to bf16): its own distance from float64 is 2 - 3.3e-3 relative L2 and <= 8.2e-3 of scale max-abs, a quarter of
the bounds, at every shape here; a failing check reports the model's distance at its shape next to the kernel's.

Bounds that differ from the five above: none.  Measured on an MI355X over every case of this file: relative L2 <= 2.4e-3
(o) and <= 3.5e-3 (gradients), max-abs <= 0.3 of its bound - the rounding model's level at every head_dim and token count;
lse <= 2e-6 except on the attn80 one-shot forward (head_dim 80, T <= 258), whose row sum comes out of the matrix pipe
(the sum of the bf16-rounded P; at most 2^-9 / ln 2 = 2.8e-3 off in the worst case): 7e-4 .. 1.6e-3 there, largest at
T = 32 and 37, against 7e-7 for the online-softmax forward on the same inputs.
"""
import contextlib
import functools
import math
import os
import sys

import pytest
import torch

from test_attn_plan_host import PAIR, SINGLE, expected, labels       # the literal table: imports without the built library

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")

HDS = (16, 32, 48, 64, 80, 96, 112, 128)
TS = (1, 31, 32, 33, 64, 65, 96, 129, 192, 193, 256, 257, 258, 259, 261, 288, 289, 319, 320)
SENTINEL = -24576.0                      # exact in bf16; no attention output of these inputs comes near it


# ---- the routing table: test ids and the coverage check ----------------------------------------------------------------

def test_sweep_reaches_every_kernel_a_resident_shape_can_reach():
    """TS holds, for every head_dim, a token count for each kernel that some T <= 320 runs at that head_dim - by the table,
    and the library plans every shape of the sweep as the table says."""
    from octic_vits_amd import _lib, ops
    for hd in HDS:
        for side in (0, 1):
            every = {labels(T, hd)[side] for T in range(1, 321)}
            assert {labels(T, hd)[side] for T in TS} == every, (hd, side)
        for T in TS:                                                # the library, and the Python side's launch names and phase plan
            assert _lib.attn_plan(T, hd) == expected(T, hd), (T, hd)
            assert ops.attn_streams(T, hd) == (labels(T, hd)[0] == "stream"), (T, hd)
            assert ops.attn_streams(T, hd, backward=True) == (labels(T, hd)[1] == "stream"), (T, hd)
            assert (ops._attn_bwd_phases(T, hd)[0][0] == 3) == (labels(T, hd)[1] == "attn80_bwd"), (T, hd)
    assert [labels(T, 80, "LEGACY")[0] for T in (37, 197, 257, 258)] == ["persist"] * 3 + ["fwd640w9"]
    assert {labels(T, 80, "BWD_PAIR")[1] for T in (37, 197, 257, 258)} == {"pair512", "pair512tile9"}


# ---- references -----------------------------------------------------------------------------------------------

def _ref64(q, k, v, do, scale):
    """float64 softmax attention (and its autograd gradients where do is given) on CPU tensors."""
    q, k, v = (t.double().requires_grad_(do is not None) for t in (q, k, v))
    s = (q @ k.transpose(-1, -2)) * scale
    o = torch.softmax(s, dim=-1) @ v
    ref = {"o": o.detach(), "lse": torch.logsumexp(s.detach(), dim=-1) / math.log(2.0)}
    if do is not None:
        o.backward(do.double())
        ref.update(dq=q.grad, dk=k.grad, dv=v.grad)
    return ref


def _rounding_model(q, k, v, do, scale):
    """float64 attention with only the kernels' roundings: P (unnormalised in the forward, recomputed from the
    log-sum-exp in the backward) and dS rounded to bf16 before the products that consume them, outputs rounded to bf16.
    A pure PyTorch computation on CPU tensors - the yardstick for a bound, never the kernel."""
    def bf(x):
        return x.float().bfloat16().double()
    q, k, v, do = (t.double() for t in (q, k, v, do))
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    l = e.sum(dim=-1, keepdim=True)
    o = bf(bf(e) @ v / l)
    p = e / l
    ds = bf(p * (do @ v.transpose(-1, -2) - (do * o).sum(dim=-1, keepdim=True)))
    return {"o": o, "lse": (m + torch.log(l)).squeeze(-1) / math.log(2.0), "dv": bf(bf(p).transpose(-1, -2) @ do),
            "dq": bf(scale * (ds @ k)), "dk": bf(scale * (ds.transpose(-1, -2) @ q))}


def _figures(got, want):
    """(max-abs error, max |ref|, L2 error, L2 of ref)"""
    d = got.double() - want
    return float(d.abs().max()), float(want.abs().max()), float(d.norm()), float(want.norm())


def _inputs(B, H, T, hd, seed, qmul=1.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16) for _ in range(4))
    return q * qmul, k, v, do


@functools.lru_cache(maxsize=4)
def _case(B, H, T, hd, seed, grads=True):
    """CPU bf16 inputs and their float64 reference, computed once per shape and shared (read-only) between tests."""
    q, k, v, do = _inputs(B, H, T, hd, seed)
    return (q, k, v, do), _ref64(q, k, v, do if grads else None, hd ** -0.5)


def _check(got, ref, T, inputs=None, names=("o", "lse", "dq", "dk", "dv"), what=""):
    """The five project bounds on every tensor in `names`: whole, on the rows of the last (partial) tile, and on rows
    256: where a ninth tile exists.  Prints every figure; collects every miss before it fails."""
    t0 = 32 * ((T - 1) // 32)
    slices = [("all", slice(None)), ("last tile", slice(t0, None))] + ([("rows 256:", slice(256, None))] if T > 256 else [])
    bad = []
    for name in names:
        g, w = got[name].detach().double().cpu(), ref[name]
        assert torch.isfinite(g).all(), f"{what}{name}: not finite"
        for label, sl in slices:
            err, mx, l2, nrm = _figures(g[:, :, sl], w[:, :, sl])
            if name == "lse":
                ok, line = err <= 2e-3, f"max-abs {err:.2e} (bound 2e-3)"
            else:
                coef = 2e-2 if name == "o" else 3e-2
                ok = err <= coef * max(1.0, mx) and l2 < 1.2e-2 * max(nrm, 1e-3)
                line = (f"max-abs {err:.2e} (bound {coef * max(1.0, mx):.2e}), L2 {l2:.2e} of {nrm:.2e} = "
                        f"{l2 / max(nrm, 1e-3):.2e} (bound 1.2e-2)")
            print(f"{what}T={T} {name} [{label}]: {line}")
            if not ok:
                bad.append(f"{name} [{label}]: {line}")
    if bad and inputs is not None:                                  # the rounding model's own distance at this shape
        hd = inputs[0].shape[-1]
        model = _rounding_model(*inputs, hd ** -0.5)
        for name in names:
            err, mx, l2, nrm = _figures(model[name], ref[name])
            bad.append(f"rounding model {name}: max-abs {err:.2e}, L2 {l2 / max(nrm, 1e-3):.2e}")
    assert not bad, what + "; ".join(bad)


@pytest.mark.parametrize("T,hd", [(33, 16), (261, 80), (320, 128)])
def test_rounding_model_leaves_room_under_the_bounds(T, hd):
    """The model's distance from float64 is what no bf16 kernel can avoid.  Held to a third of each bound, so that
    the bounds above leave room at these shapes and "3 x the model's distance" could never exceed them."""
    inputs, ref = _case(2, 2, T, hd, 1000 * hd + T)
    model = _rounding_model(*inputs, hd ** -0.5)
    for name in ("o", "dq", "dk", "dv"):
        err, mx, l2, nrm = _figures(model[name], ref[name])
        print(f"T={T} hd={hd} model {name}: max-abs {err / max(1.0, mx):.2e} of scale, L2 {l2 / nrm:.2e}")
        assert l2 < 4e-3 * nrm and err <= (2e-2 if name == "o" else 3e-2) / 3 * max(1.0, mx), name
    assert float((model["lse"] - ref["lse"]).abs().max()) < 1e-9


# ---- launches -------------------------------------------------------------------------------------------------

def _guarded(t, fill):
    """[B, H, T + 1, hd] on the device: rows :T are t (or `fill` where t is a shape), row T of every head is `fill`."""
    if isinstance(t, torch.Tensor):
        B, H, T, hd = t.shape
        full = torch.full((B, H, T + 1, hd), fill, dtype=torch.bfloat16)
        full[:, :, :T] = t
    else:
        B, H, T, hd = t
        full = torch.full((B, H, T + 1, hd), fill, dtype=torch.bfloat16)
    return full.cuda()


def _launch(inputs, guard=False):
    """Forward and backward through ops.attn_fwd / ops.attn_bwd (the routing picks the kernels).  guard: every tensor is
    the [:, :, :T] view of a [B, H, T + 1, hd] buffer (head stride (T + 1) hd: rows stay 16-byte aligned) whose row T
    holds NaN (inputs) or SENTINEL (outputs); returns the buffers too."""
    from octic_vits_amd import ops
    shape = tuple(inputs[0].shape)
    T, scale = shape[2], shape[3] ** -0.5
    if guard:
        bufs = {n: _guarded(t, float("nan")) for n, t in zip(("q", "k", "v", "do"), inputs)}
        bufs.update({n: _guarded(shape, SENTINEL) for n in ("o", "dq", "dk", "dv")})
        q, k, v, do, o, dq, dk, dv = (bufs[n][:, :, :T] for n in ("q", "k", "v", "do", "o", "dq", "dk", "dv"))
        assert q.stride() == ((T + 1) * shape[1] * shape[3], (T + 1) * shape[3], shape[3], 1)
    else:
        bufs = None
        q, k, v, do = (t.cuda() for t in inputs)
        o, dq, dk, dv = (torch.full(shape, SENTINEL, dtype=torch.bfloat16, device="cuda") for _ in range(4))
    o2, lse = ops.attn_fwd(q, k, v, scale, out=o)
    assert o2 is o
    ops.attn_bwd(q, k, v, o, do, lse, scale, dq, dk, dv)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}, bufs


@contextlib.contextmanager
def _route(knob, value):
    """octic_route_override(knob, value) for the body; the table is process-global, so 0 comes back whatever happens."""
    from octic_vits_amd import _lib
    try:
        _lib.route_override(knob, value)
        yield
    finally:
        _lib.route_override(knob, 0)


@contextlib.contextmanager
def _bwd_fused(value):
    from octic_vits_amd import ops
    old = ops.ATTN_BWD_FUSED
    try:
        ops.ATTN_BWD_FUSED = value
        yield
    finally:
        ops.ATTN_BWD_FUSED = old


# ---- 1 + 2: every head_dim x every token edge, behind guard rows ------------------------------------------------

@pytest.mark.parametrize("T,hd", [pytest.param(T, hd, id="hd%d-T%d-%s-%s" % ((hd, T) + labels(T, hd)))
                                  for hd in HDS for T in TS])
def test_sweep_matches_fp64_behind_guard_rows(T, hd):
    """o, lse, dq, dk, dv of whatever kernel the routing picks (named in the test id) against float64, whole and on the
    rows of the last partial tile; row T of every head of q, k, v, dO is NaN - a kernel that lets a padded key or query
    row reach a result produces a non-finite output - and row T of o, dq, dk, dv must keep its sentinel bit for bit."""
    inputs, ref = _case(2, 2, T, hd, 1000 * hd + T)
    got, bufs = _launch(inputs, guard=True)
    for n in ("o", "dq", "dk", "dv"):
        row = bufs[n].view(torch.int16)[:, :, T]
        want = torch.full_like(bufs[n][:, :, T], SENTINEL).view(torch.int16)
        assert torch.equal(row, want), f"{n}: the row behind token T - 1 was written"
    for n, t in zip(("q", "k", "v", "do"), inputs):                  # (and no input was written)
        assert torch.isnan(bufs[n][:, :, T].float()).all() and torch.equal(bufs[n][:, :, :T].cpu(), t), n
    _check(got, ref, T, inputs)


# ---- 3: layouts at the new token counts --------------------------------------------------------------------------

@pytest.mark.parametrize("hd", [64, 80, 96])
@pytest.mark.parametrize("T", [261, 289, 320])
def test_strided_fused_qkv_views_at_the_new_token_counts(T, hd):
    """q, k, v as strided views of one [B, T, 3, H, hd] tensor (the standard block's layout: head stride < token stride),
    gradients into one tensor of that layout."""
    from octic_vits_amd import ops
    B, H = 2, 2
    g = torch.Generator().manual_seed(7 * T + hd)
    qkv = torch.randn(B, T, 3, H, hd, generator=g).to(torch.bfloat16)
    do = torch.randn(B, H, T, hd, generator=g).to(torch.bfloat16)
    inputs = tuple(qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3)) + (do,)
    ref = _ref64(*inputs, hd ** -0.5)
    qkv_d = qkv.cuda()
    q, k, v = (qkv_d[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    o, lse = ops.attn_fwd(q, k, v, hd ** -0.5)
    dqkv = torch.full_like(qkv_d, SENTINEL)
    dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    ops.attn_bwd(q, k, v, o, do.cuda(), lse, hd ** -0.5, dq, dk, dv)
    _check({"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}, ref, T, inputs)


@pytest.mark.parametrize("w", [10, 8])
@pytest.mark.parametrize("T", [261, 289, 320])
def test_packed_rows_at_the_new_token_counts_match_the_fp64_oracle(T, w):
    """octic_attn_{fwd,bwd}_packed against the oracle's pack_heads -> float64 attention -> unpack_heads (no HIP kernel and
    no product code in the reference leg), as test_packed_attention_matches_fp64_reference does at T = 257."""
    sys.path.insert(0, ROOT)
    from oracle import octic_ref as R
    from octic_vits_amd import ops
    B, H = 2, 2
    c, hd = w * H, 8 * w
    cv = 3 * c
    g = torch.Generator().manual_seed(11 * T + w)
    qkv = (torch.randn(B, T, 3 * 8 * c, generator=g) * 0.7).to(torch.bfloat16)
    do = torch.randn(B, T, 8 * c, generator=g).to(torch.bfloat16)
    assert ops.attn_packed_ok(T, c, H, qkv.dtype)
    qkv_d, do_d = qkv.cuda(), do.cuda()
    o = torch.full((B, T, 8 * c), SENTINEL, dtype=torch.bfloat16, device="cuda")
    o, lse = ops.attn_fwd_packed(qkv_d, H, c, hd ** -0.5, out=o)
    dqkv = ops.attn_bwd_packed(qkv_d, o, do_d, lse, H, c, hd ** -0.5, out=torch.full_like(qkv_d, SENTINEL))

    x = qkv.double().requires_grad_(True)
    tup = tuple(x[..., i * cv:(i + 1) * cv] for i in range(4)) + (x[..., 4 * cv:].reshape(B, T, 2, 2 * cv),)
    q, k, v = R.pack_heads(tup, H)
    s = q @ k.transpose(-1, -2) * hd ** -0.5
    out5 = R.unpack_heads(torch.softmax(s, -1) @ v)
    ref_o = torch.cat(list(out5[:4]) + [out5[4].flatten(-2)], dim=-1)
    (ref_g,) = torch.autograd.grad(ref_o, x, do.double())
    ref = {"o": ref_o.detach().unsqueeze(1), "lse": torch.logsumexp(s.detach(), -1) / math.log(2.0),
           "dq": ref_g.unsqueeze(1)}
    # ([B, 1, T, channels]: _check slices tokens on dim 2; "dq" carries dq | dk | dv under the gradient bound)
    _check({"o": o.unsqueeze(1), "lse": lse, "dq": dqkv.unsqueeze(1)}, ref, T, names=("o", "lse", "dq"))


# ---- 4: sharp softmax through the 9- and 10-wave forward -----------------------------------------------------------

@pytest.mark.parametrize("T,hd", [(261, 80), (320, 64), (289, 96)])
def test_forward_with_large_logits_at_the_new_token_counts(T, hd):
    """q * 20: exp2(x - m) spans the whole range, the running-max rescale of fwd_pass matters.  Forward only (the
    rounding model's own gradient error is 6.8e-3 relative L2 here); the bound of test_attn_fwd_large_logits_are_stable."""
    from octic_vits_amd import ops
    q, k, v, _ = _inputs(2, 2, T, hd, 3 * T + hd, qmul=20.0)
    ref = _ref64(q, k, v, None, hd ** -0.5)
    o, lse = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), hd ** -0.5)
    o = o.double().cpu()
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    print(f"T={T} hd={hd}: max-abs {float((o - ref['o']).abs().max()):.2e}")
    assert torch.allclose(o, ref["o"], atol=3e-2, rtol=3e-2), (o - ref["o"]).abs().max()


# ---- 5: more (batch, head) units than CUs on the persistent forward at head_dim 64 --------------------------------

@pytest.mark.parametrize("T", [197, 257, 258])
def test_persistent_forward_at_head_dim_64_walks_over_several_heads(T):
    """272 units on 256 CUs: attn_fwd_persist_kernel<4, 2> fetches the next head (K by LDS-DMA, V and Q in registers)
    while it computes the current one; at T = 257 / 258 with one / two rows in the shared ninth tile."""
    from octic_vits_amd import ops
    B, H, hd = 17, 16, 64
    assert labels(T, hd)[0] == "persist"
    (q, k, v, _), ref = _case(B, H, T, hd, T, grads=False)
    o, lse = ops.attn_fwd(q.cuda(), k.cuda(), v.cuda(), hd ** -0.5)
    _check({"o": o, "lse": lse}, ref, T, names=("o", "lse"))


# ---- 6: the three attention route knobs -----------------------------------------------------------------------------

KNOB_TS = [37, 197, 257, 258]


def _knob_case(T):
    return _case(3, 16, T, 80, 80 + T)


@pytest.mark.parametrize("T", KNOB_TS)
def test_route_attn_legacy_at_head_dim_80(T):
    """ROUTE_ATTN_LEGACY = 1: attn_fwd_persist_kernel<5, 3> and the dq + dkv pair (phase 3: both in one call) where the
    default is csrc/attn80*.hip (T = 258: the ninth tile's two rows no longer fit beside the images - nine waves)."""
    from octic_vits_amd import _lib
    inputs, ref = _knob_case(T)
    with _route(_lib.ROUTE_ATTN_LEGACY, 1):
        got, _ = _launch(inputs)
    assert _lib.route_override(_lib.ROUTE_ATTN_LEGACY, 0) == 0
    _check(got, ref, T, inputs)


@pytest.mark.parametrize("T", KNOB_TS)
def test_route_attn_online_at_head_dim_80(T):
    """ROUTE_ATTN_ONLINE = 1: the attn80 online-softmax forward against float64 and against the default one-shot one."""
    from octic_vits_amd import _lib, ops
    inputs, ref = _knob_case(T)
    q, k, v = (t.cuda() for t in inputs[:3])
    with _route(_lib.ROUTE_ATTN_ONLINE, 1):
        o1, lse1 = ops.attn_fwd(q, k, v, 80 ** -0.5)
    assert _lib.route_override(_lib.ROUTE_ATTN_ONLINE, 0) == 0
    o0, lse0 = ops.attn_fwd(q, k, v, 80 ** -0.5)
    _check({"o": o1, "lse": lse1}, ref, T, names=("o", "lse"), what="online ")
    _check({"o": o0, "lse": lse0}, ref, T, names=("o", "lse"), what="one-shot ")
    _check({"o": o1, "lse": lse1}, {"o": o0.double().cpu(), "lse": lse0.double().cpu()}, T, names=("o", "lse"),
           what="online vs one-shot ")


@pytest.mark.parametrize("T", KNOB_TS)
def test_route_attn_bwd_pair_at_head_dim_80(T):
    """ROUTE_ATTN_BWD_PAIR = 1: a phase-3 call to the C entry point (ops plans no such call under the knob: it names the dq
    and dkv kernels and sends two) runs dq then dkv in that one call - the same two kernels as the two calls of ops.attn_bwd,
    so bit-identical to them."""
    from octic_vits_amd import _lib, ops
    inputs, ref = _knob_case(T)
    scale = 80 ** -0.5
    with _bwd_fused(True), _route(_lib.ROUTE_ATTN_BWD_PAIR, 1):
        for t in KNOB_TS:
            assert [p[:2] for p in ops._attn_bwd_phases(t, 80)] == [(1, "attn_bwd_dq_kernel"), (2, "attn_bwd_dkv_kernel")]
        two, _ = _launch(inputs)                                     # phase 1, then phase 2
        q, k, v, do = (t.cuda() for t in inputs)
        dq, dk, dv = (torch.full_like(q, SENTINEL) for _ in range(3))
        delta = torch.empty(q.shape[:3], dtype=torch.float32, device="cuda")
        st = q.stride()
        _lib.check(_lib.lib().octic_attn_bwd(*(ops._p(t) for t in (q, k, v, two["o"], do, two["lse"], delta, dq, dk, dv)),
                                             *q.shape, *(st[:3] * 3), scale, 3, ops._stream(q)))
        torch.cuda.synchronize()
    assert _lib.route_override(_lib.ROUTE_ATTN_BWD_PAIR, 0) == 0
    got = dict(two, dq=dq, dk=dk, dv=dv)
    _check(got, ref, T, inputs)
    for n in ("dq", "dk", "dv"):
        assert torch.equal(got[n], two[n]), f"{n}: one call with phase 3 differs from the two calls"
    with _bwd_fused(False):                                         # and the two calls of ATTN_BWD_FUSED = False, knob at 0
        unfused, _ = _launch(inputs)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(unfused[n], two[n]), f"{n}: the pair under the knob differs from the pair without it"


# ---- 7: repeatability -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hd", [64, 80, 128])
@pytest.mark.parametrize("T", [261, 320])
def test_two_launches_are_bitwise_equal(T, hd):
    """No atomics, fixed summation orders (the shared tile's partials are summed wave 0 .. W - 1): two launches agree
    bit for bit, forward and backward."""
    inputs = _inputs(2, 2, T, hd, T + hd)
    one, _ = _launch(inputs)
    two, _ = _launch(inputs)
    for n in ("o", "lse", "dq", "dk", "dv"):
        assert torch.equal(one[n], two[n]), n


# ---- 8: KERNEL_TIMER books what the plan says ----------------------------------------------------------------------------

_FWD_TIMER = {"stream": "attn_fwd_stream_kernel"}
_BWD_TIMER = {"attn80_bwd": ["attn_bwd_kernel"], "stream": ["attn_bwd_dq_stream_kernel", "attn_bwd_dkv_stream_kernel"]}


@pytest.mark.parametrize("T,hd,knob", [(37, 80, None), (257, 80, None), (258, 80, None), (289, 112, None), (257, 128, None),
                                       (257, 80, "STREAM"), (257, 80, "LEGACY"), (257, 80, "BWD_PAIR"), (257, 80, "ONLINE")])
def test_kernel_timer_names_what_the_plan_says(T, hd, knob):
    """The launches ops.attn_fwd / ops.attn_bwd book in KERNEL_TIMER, and their FLOP, are those of the library's plan - under
    the knobs too (ROUTE_ATTN_LEGACY / ROUTE_ATTN_BWD_PAIR: two calls booked as dq and dkv at 14 T^2 hd, where a single
    phase-3 call used to be booked as the single-pass kernel at 10)."""
    from octic_vits_amd import _lib, ops
    f, b = labels(T, hd, knob)
    want = [_FWD_TIMER.get(f, "attn_fwd_kernel")] + _BWD_TIMER.get(b, ["attn_bwd_dq_kernel", "attn_bwd_dkv_kernel"])
    inputs = _inputs(2, 2, T, hd, T + hd)
    try:
        if knob:
            _lib.route_override(getattr(_lib, "ROUTE_ATTN_" + knob), 1)
        plan = _lib.attn_plan(T, hd)
        ops.KERNEL_TIMER.enable()
        _launch(inputs)
        records = list(ops.KERNEL_TIMER.records)
    finally:
        ops.KERNEL_TIMER.disable()
        if knob:
            _lib.route_override(getattr(_lib, "ROUTE_ATTN_" + knob), 0)
    assert plan == expected(T, hd, knob)
    assert [r[0] for r in records] == want
    unit = 2 * 2 * T * T * hd
    assert [r[4] / unit for r in records] == [4.0] + ([10.0] if plan[2] == SINGLE else [6.0, 8.0])
    assert (plan[2] == SINGLE) == (b == "attn80_bwd") and (plan[2] == PAIR) == b.startswith("pair")
