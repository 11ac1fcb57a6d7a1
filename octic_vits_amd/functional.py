"""Autograd wrappers of the HIP engine (the PyTorch-ROCm custom-op surface).

Every hot op of the octic block is one ``torch.autograd.Function`` whose forward AND backward are
launches of hand-written gfx950 kernels through the C ABI (``ops.py`` → ``liboctic_hip.so``).
The engine's native tensor is the *packed* token row ``[B, T, 8c] = [A1|A2|B1|B2|E_row0|E_row1]``;
``Octic`` wraps it as the reference's 5-tuple (zero-copy views) so modules stay drop-in.

Precision follows the caller like the reference does: plain fp32 tensors run the exact-f32 MFMA
path (used for the reference's fp32 equivariance tolerances); under
``torch.autocast('cuda', dtype=torch.bfloat16)`` linears/GELU/attention run in bf16 with f32
accumulation while the residual stream, LayerNorm statistics and parameter gradients stay f32
(that is what autocast does to the reference).
"""
import os

import torch

from . import ops


class Octic(tuple):
    """The reference's 5-tuple (A1,A2,B1,B2:[B,T,c]; E:[B,T,2,2c]) as views of one packed tensor."""

    def __new__(cls, packed: torch.Tensor, c: int):
        self = super().__new__(cls, ops.split_packed(packed, c))
        self.packed, self.c = packed, c
        return self


def as_packed(xs):
    """Packed [.., 8c] tensor of an Octic (free) or of any reference-style 5-tuple (one torch.cat)."""
    if isinstance(xs, Octic):
        return xs.packed, xs.c
    if len(xs) != 5:
        raise AssertionError("Input should be a 5-tuple")
    c = xs[0].shape[-1]
    if xs[4].shape[-2:] != (2, 2 * c):
        raise ValueError(f"E irrep must be [..., 2, {2 * c}], got {tuple(xs[4].shape)}")
    return torch.cat([xs[0], xs[1], xs[2], xs[3], xs[4].flatten(-2)], dim=-1), c


_FP16_NOTE = [False]


ATTN_PACKED = True     # AttentionD8: attention kernels read / write the packed irrep rows (no pack / unpack passes)
RAGGED = None          # ragged.Ragged of the [1, R, .] tensor the blocks are looking at (several crop sets as one row tensor:
                       # set by dinov2_models' block loop, consulted by the attention modules), or None


def compute_dtype(t: torch.Tensor):
    """Operand dtype of the octic kernels for `t` under the ambient autocast state.  bf16 autocast -> bf16 (the fast
    path, BASELINE dtype).  fp16 autocast (the reference's DeiT default, deit/engine.py:56) -> float32: the engine has no
    fp16 kernels, so the octic half runs on its exact-f32 MFMA path - a superset of fp16's precision, slower than bf16 -
    and its attention is on the engine too (octic_attn_*_f32, csrc/attn_f32.hip); the standard blocks run the
    reference's own eager fp16 ops.  Said once on stderr, never silently."""
    if torch.is_autocast_enabled("cuda"):
        dt = torch.get_autocast_dtype("cuda")
        if dt == torch.bfloat16:
            return dt
        if dt == torch.float16:
            if not _FP16_NOTE[0]:
                _FP16_NOTE[0] = True
                import sys
                print("octic engine: fp16 autocast -> the octic blocks compute in float32 (no fp16 kernels; use "
                      "dtype=torch.bfloat16 for the fast path)", file=sys.stderr)
            if t.dtype not in (torch.float32, torch.float16):
                raise TypeError(f"octic engine under fp16 autocast expects float32 / float16 inputs, got {t.dtype}")
            return torch.float32
        raise NotImplementedError(f"octic engine: autocast dtype {dt} is not supported (bfloat16 or float16)")
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"octic engine supports float32 / bfloat16, got {t.dtype}")
    return t.dtype


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


# ------------------------------------------------------------------------------------------- GELU
class GeluD8PackedFn(torch.autograd.Function):
    """D8-GELU on packed rows.  sample_scale / rps (linear_skip_scale): the stochastic-depth factor of the MLP branch the node
    sits in, one entry per sample of rps rows.  The kernels then read no row of a dropped sample and write +0 there, in the
    forward and in the backward (include/octic_hip.h: octic_gelu_d8_*_skip) - the readers of both results (fc2 and its
    weight gradient; fc1's input and weight gradients) multiply those rows by zero anyway."""

    @staticmethod
    def forward(ctx, x, c, sample_scale=None, rps=0):
        x = _c(x)
        y = torch.empty_like(x)
        M = x.numel() // (8 * c)
        ss = linear_skip_scale(sample_scale, rps, M)
        ops.gelu_fwd(ops.pview(x, c), ops.pview(y, c), M, c, x.dtype, x, sample_scale=ss, rows_per_sample=rps)
        ctx.save_for_backward(x, ss)
        ctx.c, ctx.rps = c, rps
        return y

    @staticmethod
    def backward(ctx, g):
        x, ss = ctx.saved_tensors
        c = ctx.c
        g = _c(g.to(x.dtype))
        gi = torch.empty_like(x)
        ops.gelu_bwd(ops.pview(g, c), ops.pview(x, c), ops.pview(gi, c), x.numel() // (8 * c), c, x.dtype, x,
                     sample_scale=ss, rows_per_sample=ctx.rps)
        return gi, None, None, None


class GeluD8Function(torch.autograd.Function):
    """Drop-in for the reference's one custom-op boundary ``TritonGeluD8Function`` (d8_gelu.py:456-478):
    five separate tensors in, five out; strides are handed to the kernel, nothing is repacked."""

    @staticmethod
    def forward(ctx, x_A1, x_A2, x_B1, x_B2, x_2d):
        xs = tuple(_c(t) for t in (x_A1, x_A2, x_B1, x_B2, x_2d))
        c = xs[0].shape[-1]
        ys = tuple(torch.empty_like(t) for t in xs)
        M = xs[0].numel() // c
        xv, k1 = ops.tview(xs, c)
        yv, k2 = ops.tview(ys, c)
        ops.gelu_fwd(xv, yv, M, c, xs[0].dtype, xs[0])
        ctx.save_for_backward(*xs)
        return ys

    @staticmethod
    def backward(ctx, *gs):
        xs = ctx.saved_tensors
        c = xs[0].shape[-1]
        gs = tuple(_c(g.to(xs[0].dtype)) for g in gs)
        outs = tuple(torch.empty_like(t) for t in xs)
        gv, k1 = ops.tview(gs, c)
        xv, k2 = ops.tview(xs, c)
        ov, k3 = ops.tview(outs, c)
        ops.gelu_bwd(gv, xv, ov, xs[0].numel() // c, c, xs[0].dtype, xs[0])
        return outs


# ------------------------------------------------------------------------------------- LayerNorm
class LayerNormD8Fn(torch.autograd.Function):
    """Returns (y, x): the second output is the input stream itself.  A block that takes its residual connection
    from it gets the residual cotangent added inside the backward kernel (no separate accumulation pass)."""

    @staticmethod
    def forward(ctx, x, a1, a2, b1, b2, ae, beta, eps, c, out_dtype):
        xin = x
        x = _c(x.float())
        alpha = None if a1 is None else [_c(t.float()) for t in (a1, a2, b1, b2, ae)]
        y, stats = ops.layernorm_fwd(x, alpha, None if beta is None else _c(beta.float()), eps, out_dtype, c)
        ctx.save_for_backward(x, stats, *(alpha or []))
        ctx.c, ctx.has_affine, ctx.has_beta = c, alpha is not None, beta is not None
        ctx.set_materialize_grads(False)
        row_skip_attach(ctx, y)
        return y, xin.view_as(xin)

    @staticmethod
    def backward(ctx, g, gres):
        x, stats, *alpha = ctx.saved_tensors
        if g is None:
            return (gres,) + (None,) * 9
        alpha = alpha if ctx.has_affine else None
        dres = None if gres is None else _c(gres.float())
        ns, nrps = row_skip_get(ctx, x.numel() // (8 * ctx.c))
        dx, dal, dbeta = ops.layernorm_bwd(_c(g), x, stats, alpha, dres, ctx.c, want_param_grads=ctx.has_affine,
                                           sample_scale=ns, rows_per_sample=nrps)
        if dal is None:
            dal = [None] * 5
        return (dx, *dal, dbeta if ctx.has_beta else None, None, None, None)


# ---------------------------------------------------------------------------------------- Linear
class WeightPrep:
    """Compute-dtype copies of a LinearD8's weights: ``wb`` for the forward GEMM and ``wt`` — transposed,
    with the layer-scale folded in — for the input-gradient GEMM (dX = dY·diag(cs)·W)."""

    def __init__(self):
        self.key = None
        self.wb = self.wt = None
        self.last = None            # (w5, cs5, dtype, cin, cout) of the latest call: what a PrepBatch needs
        self.flat = None            # (wb, wt) flat bf16 buffers a PrepBatch refreshes IN PLACE after every optimizer step: what a
                                    # traced graph may read as plain inputs (dispatch.py) - None while this object prepares itself

    @staticmethod
    def _key(w5, cs5, dtype):
        return (dtype, tuple((w.data_ptr(), w._version) for w in w5),
                None if cs5 is None else tuple((s.data_ptr(), s._version) for s in cs5))

    def get(self, w5, cs5, dtype, cin, cout):
        key = self._key(w5, cs5, dtype)
        if key != self.key:
            with torch.no_grad():
                w32 = [_c(w.detach().float()) for w in w5]
                cs32 = None if cs5 is None else [_c(s.detach().float()) for s in cs5]
                wb, self.wt = ops.linear_prep(w32, cs32, cin, cout, dtype, want_wb=(dtype != torch.float32))
                self.wb = wb if wb is not None else w32   # f32: the master weights are the forward operand
            self.key = key
            self.flat = None
        self.last = (w5, cs5, dtype, cin, cout)
        return self.wb, self.wt

    def adopt(self, wb, wt, flat=None):
        """Copies produced elsewhere (PrepBatch) are current for the parameters' present versions."""
        w5, cs5, dtype, _, _ = self.last
        self.wb, self.wt = wb, wt
        self.key = self._key(w5, cs5, dtype)
        self.flat = flat


class PrepBatch:
    """All bf16 LinearD8 weight preparations of a model in ONE launch (octic_linear_d8_prep_batch), run by the fused
    optimizer right after its update instead of 64 per-layer launches at the next forward."""

    def __init__(self, preps):
        import numpy as np
        self.preps = [p for p in preps if p.last is not None and p.last[2] == torch.bfloat16
                      and all(t.dtype == torch.float32 and t.is_contiguous() for t in p.last[0])
                      and (p.last[1] is None or all(t.dtype == torch.float32 and t.is_contiguous() for t in p.last[1]))]
        if not self.preps:
            self.items = None
            return
        dev = self.preps[0].last[0][0].device
        dt = np.dtype([("w", "<u8", 5), ("cs", "<u8", 5), ("wb", "<u8"), ("wt", "<u8"), ("cin", "<i4"), ("cout", "<i4"),
                       ("block_begin", "<i4"), ("block_count", "<i4")])
        tab = np.zeros(len(self.preps), dtype=dt)
        self.bufs, self.flats, blocks = [], [], 0
        for i, p in enumerate(self.preps):
            w5, cs5, dtype, cin, cout = p.last
            n = 8 * cin * cout
            wb = torch.empty(n, dtype=dtype, device=dev)
            wt = torch.empty(n, dtype=dtype, device=dev)
            self.bufs.append((ops.prep_views(wb, cin, cout, False), ops.prep_views(wt, cin, cout, True)))
            self.flats.append((wb, wt))
            cnt = ops.lib().octic_linear_d8_prep_batch_blocks(cin, cout)   # one 64 x 64 tile per workgroup
            tab[i]["w"] = [t.data_ptr() for t in w5]
            tab[i]["cs"] = [0] * 5 if cs5 is None else [t.data_ptr() for t in cs5]
            tab[i]["wb"], tab[i]["wt"] = wb.data_ptr(), wt.data_ptr()
            tab[i]["cin"], tab[i]["cout"] = cin, cout
            tab[i]["block_begin"], tab[i]["block_count"] = blocks, cnt
            blocks += cnt
        self.total_blocks = blocks
        self.items = torch.from_numpy(tab.view(np.uint8).copy()).to(dev)
        self._keep = [p.last for p in self.preps]        # the parameters whose addresses are in the table
        self._ptrs = self._current_ptrs()

    def _current_ptrs(self):
        return tuple(t.data_ptr() for p in self.preps for t in (tuple(p.last[0]) + tuple(p.last[1] or ())))

    def stale(self):
        """True when a parameter was re-allocated since the table was built (the table holds raw addresses)."""
        return self.items is not None and self._current_ptrs() != self._ptrs

    def run(self):
        if self.items is None:
            return
        ops.check(ops.lib().octic_linear_d8_prep_batch(ops._p(self.items), len(self.preps), self.total_blocks,
                                                       ops.dt_code(torch.bfloat16), ops._stream(self.items)))
        for p, (wb, wt), flat in zip(self.preps, self.bufs, self.flats):
            p.adopt(wb, wt, flat)


def _linear_d8_fwd_prep(ctx, x, w5, cs5, bias, rs, cin, cout, rps, dtype, out_dtype, prep):
    """What both LinearD8 nodes do in front of their forward launch: x in the compute dtype, the prepared weights, f32 copies of
    bias / layer scale / row scale and the output to fill.  Leaves on ctx what _linear_d8_grads reads back (ctx.lin).
    Returns (x, forward weights, M, y, b32, cs32, rs32)."""
    ops._require_cuda(x)
    x_in_dtype = x.dtype
    if x.dtype != dtype:
        x = ops.cast_rowscale(_c(x.float()), None, 1, dtype, cin)
    x = _c(x)
    wb, wt = prep.get(w5, cs5, dtype, cin, cout)
    M = x.numel() // (8 * cin)
    y = torch.empty(x.shape[:-1] + (8 * cout,), dtype=out_dtype, device=x.device)
    b32 = None if bias is None else _c(bias.detach().float())
    cs32 = None if cs5 is None else [_c(s.detach().float()) for s in cs5]
    rs32 = None if rs is None else _c(rs.float())
    ctx.lin = (cin, cout, rps, dtype, cs5 is not None, bias is not None, x_in_dtype, wt)
    return x, wb, M, y, b32, cs32, rs32


def _linear_d8_grads(ctx, x, g, w5, cs32, b32, ss_dx, z_dx=None, ss_dw=None):
    """The gradient half of both LinearD8 nodes' backward, from g = the cotangent of the branch in the compute dtype: the
    input-gradient launch under its masks (ss_dx / z_dx: LinearD8Fn.forward), the bias column sums and the weight gradients
    (ss_dw: linear_wgrad_skip_scale - the rows of g are zero for the samples it drops; f32 masters only).
    Returns (dx or None, dw5, dbias, dcs5)."""
    cin, cout, rps, dtype, has_cs, has_bias, x_in_dtype, wt = ctx.lin
    M = x.numel() // (8 * cin)
    gv, xv = ops.pview(g, cout), ops.pview(x, cin)
    dx = None
    if ctx.needs_input_grad[0]:
        dx = torch.empty(x.shape, dtype=dtype, device=x.device)
        ops.linear_fwd(gv, wt, None, ops.pview(dx, cin), M, cout, cin, dtype, dtype, x, sample_scale=ss_dx, skip_rps=rps,
                       dropped=z_dx, dropped_rps=rps)
        if dx.dtype != x_in_dtype:
            dx = dx.to(x_in_dtype)
    # bias gradient = column sums of the invariant block of g: the bf16 wgrad kernel produces them on the side
    # (one extra MFMA row); other paths run the column-sum kernel
    dysum = ops.colsum_a1(gv, M, cout, dtype, x) if (has_bias and not ops.wgrad_has_colsum(cin, cout, dtype)) else None
    w32 = [_c(w.detach().float()) for w in w5] if has_cs else None
    f32_masters = all(w.dtype == torch.float32 for w in w5)      # else the casts below read dw at once: no deferral
    dw, dcs, dbias = ops.linear_wgrad(xv, gv, M, cin, cout, dtype, x, w32=w32, cs5=cs32, bias=b32, dysum=dysum,
                                      want_bias=has_bias, may_defer=f32_masters, wparams=w5 if f32_masters else None,
                                      sample_scale=ss_dw if f32_masters else None, rows_per_sample=rps)
    if not f32_masters:
        dw = [d.to(w.dtype) for d, w in zip(dw, w5)]
    return dx, dw, dbias, (dcs if has_cs else [None] * 5)


class LinearD8Fn(torch.autograd.Function):
    """y = resid + rs*cs*(x W^T + b)   (resid / rs / cs optional).  See octic_hip.h for the math."""

    @staticmethod
    def forward(ctx, x, wA1, wA2, wB1, wB2, wE, bias, resid, rs, sA1, sA2, sB1, sB2, sE, cin, cout, rps, dtype, prep,
                skip_out=None, skip_dx=None, zero_dx=None, zero_dy=None):
        """skip_out / skip_dx: the stochastic-depth factor of the branch this layer sits in, as the sample mask of the forward
        launch / of the input-gradient launch - given by the caller only where EVERY reader of that launch's output honours the
        same mask (linear_skip_scale; DESIGN.md 'Routing rules').  The rows of a dropped sample may then stay unwritten.
        zero_dx: the same factor as the `dropped` mask of a plain layer's input-gradient launch (ring_skip_scale) - given only
        where the cotangent rows of a dropped sample are exactly zero; every row of dx is written (zeros there).  A fused
        forward hands its own rs to the launch as `dropped`: the tail multiplies those samples' rows by 0.
        zero_dy: the factor of the branch where the cotangent rows of THIS layer's output are exactly zero for a dropped
        sample, as the mask of the weight gradient (linear_wgrad_skip_scale) - the layer's own rs, or the caller's promise
        for a plain layer; it asks no skip switch, so both arms of a bitwise comparison sum alike."""
        w5 = (wA1, wA2, wB1, wB2, wE)
        cs5 = None if sA1 is None else (sA1, sA2, sB1, sB2, sE)
        fused = resid is not None
        out_dtype = resid.dtype if fused else dtype
        handed = x
        x, wb, M, y, b32, cs32, rs32 = _linear_d8_fwd_prep(ctx, x, w5, cs5, bias, rs, cin, cout, rps, dtype, out_dtype, prep)
        rv = ops.pview(_c(resid), cout) if fused else None
        plain = not fused and rs32 is None and cs32 is None
        ss_out = linear_skip_scale(skip_out, rps, M) if plain else None
        dropped = ring_skip_scale(rs32, rps, M) if fused else None
        ops.linear_fwd(ops.pview(x, cin), wb, b32, ops.pview(y, cout), M, cin, cout, dtype, out_dtype, x,
                       resid_v=rv, rs=rs32, rps=rps, cs5=cs32, sample_scale=ss_out, skip_rps=rps, dropped=dropped, dropped_rps=rps)
        ss_dx = linear_skip_scale(skip_dx, rps, M)
        z_dx = ring_skip_scale(zero_dx, rps, M) if (plain and ss_dx is None) else None
        # zero cotangent rows in, zero dx rows out (computed or stored, every row written): the norm in front may skip them
        row_skip_fill(handed, row_skip_scale(zero_dx, rps, M) if (plain and ss_dx is None) else None, rps, M)
        ss_dw = linear_wgrad_skip_scale(rs32 if (rs is not None and zero_dy is rs) else zero_dy, rps, M)
        ctx.save_for_backward(x, rs32, b32, ss_dx, z_dx, ss_dw, *w5, *(cs32 or []))
        ctx.fused = fused
        return y

    @staticmethod
    def backward(ctx, dy):
        cin, cout, rps, dtype, has_cs = ctx.lin[:5]
        x, rs32, b32, ss_dx, z_dx, ss_dw, *rest = ctx.saved_tensors
        w5, cs32 = rest[:5], (rest[5:] if has_cs else None)
        dy = _c(dy)
        if ctx.fused or rs32 is not None or dy.dtype != dtype:
            g = ops.cast_rowscale(_c(dy.float()), rs32, rps, dtype, cout)  # cotangent of the branch
        else:
            g = dy
        dx, dw, dbias, dcs = _linear_d8_grads(ctx, x, g, w5, cs32, b32, ss_dx, z_dx, ss_dw)
        return (dx, *dw, dbias, dy if ctx.fused else None, None, *dcs, None, None, None, None, None, None, None, None, None)


class LinearD8NormFn(torch.autograd.Function):
    """LinearD8Fn with the fused residual tail (y = resid + rs*cs*(x W^T + b), the new f32 stream) followed by the
    LayerNormD8 that opens the NEXT branch: returns (y, LayerNorm(y)).  The forward is the two kernels one after the other
    (the GEMM epilogue owns column slices, not rows); the point is the backward: the norm's backward kernel, which
    produces the stream cotangent dx anyway, also stores bf16(rs * dx) - the cotangent of this layer's branch - so the
    cast_rowscale pass over dx disappears (functional.OCTIC_NEXT_NORM)."""

    @staticmethod
    def forward(ctx, x, wA1, wA2, wB1, wB2, wE, bias, resid, rs, sA1, sA2, sB1, sB2, sE, cin, cout, rps, dtype, prep,
                a1, a2, b1, b2, ae, beta, eps, skip_dx=None, zero_dy=None):
        """skip_dx: as in LinearD8Fn (the sample mask of the input-gradient launch).  The fused forward hands rs to the launch as
        its `dropped` mask (ring_skip_scale).  zero_dy: as in LinearD8Fn (the layer's own rs as the weight gradient's mask)."""
        w5 = (wA1, wA2, wB1, wB2, wE)
        cs5 = None if sA1 is None else (sA1, sA2, sB1, sB2, sE)
        x, wb, M, y, b32, cs32, rs32 = _linear_d8_fwd_prep(ctx, x, w5, cs5, bias, rs, cin, cout, rps, dtype, resid.dtype, prep)
        ops.linear_fwd(ops.pview(x, cin), wb, b32, ops.pview(y, cout), M, cin, cout, dtype, resid.dtype, x,
                       resid_v=ops.pview(_c(resid), cout), rs=rs32, rps=rps, cs5=cs32, dropped=ring_skip_scale(rs32, rps, M),
                       dropped_rps=rps)
        alpha = None if a1 is None else [_c(t.float()) for t in (a1, a2, b1, b2, ae)]
        yn, stats = ops.layernorm_fwd(y, alpha, None if beta is None else _c(beta.float()), eps, dtype, cout)
        ss_dw = linear_wgrad_skip_scale(rs32 if (rs is not None and zero_dy is rs) else zero_dy, rps, M)
        ctx.save_for_backward(x, rs32, b32, y, stats, linear_skip_scale(skip_dx, rps, M), ss_dw, *w5, *(cs32 or []),
                              *(alpha or []))
        ctx.has_affine, ctx.has_beta = alpha is not None, beta is not None
        ctx.set_materialize_grads(False)
        row_skip_attach(ctx, yn)
        return y, yn

    @staticmethod
    def backward(ctx, dy, dyn):
        cin, cout, rps, dtype, has_cs = ctx.lin[:5]
        has_affine = ctx.has_affine
        x, rs32, b32, y, stats, ss_dx, ss_dw, *rest = ctx.saved_tensors
        w5 = rest[:5]
        cs32 = rest[5:10] if has_cs else None
        alpha = rest[(10 if has_cs else 5):] if has_affine else None
        M = x.numel() // (8 * cin)
        dal, dbeta, g = [None] * 5, None, None
        if dyn is not None:
            dres = None if dy is None else _c(dy.float())
            gn = _c(dyn)
            ns, nrps = row_skip_get(ctx, M)
            mine = dres is not None and STREAM_GRADS.take(dres)    # (always asked: the entry is this node's to consume)
            if ops.layernorm_bwd_cast_ok(gn, y, cout) and dtype == torch.bfloat16:
                dy, dal_, dbeta, g = ops.layernorm_bwd_cast(gn, y, stats, alpha, dres, cout, rs32, rps,
                                                            want_param_grads=has_affine, sample_scale=ns, rows_per_sample=nrps,
                                                            inplace=mine and ns is not None)
            else:
                dy, dal_, dbeta = ops.layernorm_bwd(gn, y, stats, alpha, dres, cout, want_param_grads=has_affine,
                                                    sample_scale=ns, rows_per_sample=nrps)
            dal = dal_ if dal_ is not None else dal
            STREAM_GRADS.offer(dy)                                 # allocated here, or the owned buffer updated in place
        dy = _c(dy)
        if g is None:
            g = ops.cast_rowscale(_c(dy.float()), rs32, rps, dtype, cout)  # cotangent of the branch
        dx, dw, dbias, dcs = _linear_d8_grads(ctx, x, g, w5, cs32, b32, ss_dx, ss_dw=ss_dw)
        return (dx, *dw, dbias, dy, None, *dcs, None, None, None, None, None, *dal, dbeta if ctx.has_beta else None, None, None,
                None)


# --------------------------------------------------------------------------------- head packing
class PackHeadsFn(torch.autograd.Function):
    """packed qkv [B,T,3*8c] -> (q, k, v) each [B,H,T,8c/H].  Three separate outputs so autograd hands the three
    SDPA gradients straight back (no zero-fill + add of a stacked [3,...] tensor)."""

    @staticmethod
    def forward(ctx, qkv, H, c):
        B, T = qkv.shape[0], qkv.shape[1]
        ctx.meta = (B, T, H, c)
        q, k, v = ops.pack_heads(_c(qkv), B, T, H, c, 3)
        return q, k, v

    @staticmethod
    def backward(ctx, gq, gk, gv):
        B, T, H, c = ctx.meta
        return ops.unpack_heads([gq, gk, gv], B, T, H, c), None, None


class UnpackHeadsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, c):
        B, H, T, _ = o.shape
        ctx.meta = (B, T, H, c)
        return ops.unpack_heads([o], B, T, H, c)

    @staticmethod
    def backward(ctx, g):
        B, T, H, c = ctx.meta
        return ops.pack_heads(_c(g), B, T, H, c, 1)[0], None


# ------------------------------------------------------------------------------------- attention
class AttnFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd)) v for separate q, k, v of shape [B,H,T,hd] (bf16, or float32 on the exact-f32 kernels of
    csrc/attn_f32.hip) — HIP forward and backward."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        q, k, v = _c(q), _c(k), _c(v)
        o, lse = ops.attn_fwd(q, k, v, scale)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        do = _c(do)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        ops.attn_bwd(q, k, v, o, do, lse, ctx.scale, dq, dk, dv)
        return dq, dk, dv, None


def _skip_from_env(name):
    """One of the OCTIC_*_SKIP switches below: on unless the variable is set to 0."""
    return os.environ.get(name, "1").strip() != "0"


# Stochastic depth: a block draws its per-sample factor rs[b] (0 or 1 / keep) BEFORE the attention branch runs and the branch's
# tail multiplies the branch output with it, so everything the softmax core computes for a dropped sample is discarded in the
# forward and meets a zero cotangent in the backward.  With ATTN_SKIP_DROPPED the factor travels to the attention kernels, which
# skip those samples where their work is dealt per (sample, head) - same launch shapes, so it lives inside a captured step
# (include/octic_hip.h: octic_attn_*_skip).  Read once at import from OCTIC_ATTN_SKIP (0 = off).
ATTN_SKIP_DROPPED = _skip_from_env("OCTIC_ATTN_SKIP")


def skip_scale(rs, B):
    """rs as the attention kernels' sample_scale: the block's per-sample factor when the switch is on and rs is one float32
    entry per sample on the GPU (not the per-row factors of a ragged row tensor, not a traced value); None otherwise."""
    if (not ATTN_SKIP_DROPPED or rs is None or not rs.is_cuda or rs.dtype != torch.float32 or rs.dim() != 1
            or rs.numel() != B or not rs.is_contiguous()):
        return None
    return rs.detach()


# The same factor makes every dY row of a dropped sample exactly zero in the branch's four weight gradients (proj and fc2: the
# tail's rs * gamma * gout; fc1: gelu' * (0 W2); qkv: the attention backward of dO = 0), so half of what csrc/dense_wgrad.hip
# reduces over multiplies zeros.  With WGRAD_SKIP_DROPPED the factor travels to the TN kernel, which leaves out the reduction
# steps that only touch dropped samples - same launch shapes, same bits (include/octic_hip.h: octic_dense_wgrad_tn_skip).
# Read once at import from OCTIC_WGRAD_SKIP (0 = off).
WGRAD_SKIP_DROPPED = _skip_from_env("OCTIC_WGRAD_SKIP")


def whole_sample_mask(rs, rps, M, rows_to=None):
    """rs as the mask of whole samples over M token rows, whichever kernel family reads it: the branch's per-sample factor when
    rs is one float32 entry per sample of rps rows on the GPU with rps * B == M; None for compact rows of a stream (rows_to),
    the per-row factors of a ragged row tensor (rps 1), a traced value, eval and drop_path 0 (rs None).  The *_skip_scale
    functions below are this behind their switches."""
    if (rs is None or rows_to is not None or torch.compiler.is_compiling() or not rs.is_cuda
            or rs.dtype != torch.float32 or rs.dim() != 1 or not rs.is_contiguous() or rps < 2 or rs.numel() * rps != M):
        return None
    return rs.detach()


def wgrad_skip_scale(rs, rps, M, rows_to=None):
    """rs as the TN kernel's sample_scale for a weight gradient over M token rows: whole_sample_mask while the switch is on."""
    return whole_sample_mask(rs, rps, M, rows_to) if WGRAD_SKIP_DROPPED else None


# The eight dense_nt_kernel launches of a standard block (csrc/dense_gemm.hip) compute rows nobody needs for a dropped sample:
# qkv's output is read by the attention kernels alone, proj's and fc2's meet rs = 0 in the residual tail, fc1's two outputs meet
# zero dY rows in fc2's gradients, and each of the four input gradients starts from a cotangent that is exactly zero for the
# sample.  With DENSE_NT_SKIP_DROPPED the branch's factor travels to the kernel as its sample_scale: row panels whose samples
# are all dropped store +0 instead of being computed, the kept rows keep their bits (include/octic_hip.h:
# octic_dense_gemm_nt_tokens_skip).  Read once at import from OCTIC_DENSE_SKIP (0 = off).
DENSE_NT_SKIP_DROPPED = _skip_from_env("OCTIC_DENSE_SKIP")


# A masked N = 1280 launch (proj, fc2, the input gradients of qkv / proj / fc1) is one round of 256 x 320 tiles, so it lasts as
# long as one live tile whatever the mask drops.  With DENSE_NARROW_DROPPED such a launch counts its live panels on the device
# and runs 256-wide tiles - shorter, and still one round - while they fit the CUs (include/octic_hip.h:
# octic_dense_gemm_nt_tokens_adaptive); same bits.  Effective only while DENSE_NT_SKIP_DROPPED is on (no mask, no choice).  Read
# once at import from OCTIC_DENSE_NARROW (0 = off).
DENSE_NARROW_DROPPED = _skip_from_env("OCTIC_DENSE_NARROW")


# Such a launch leaves the CUs of its dead tiles idle for most of its length, and its class-token rows wait behind it for one or
# two latency-bound launches of their own (dense_cls_kernel, or dense_cls_part_kernel + dense_cls_sum_kernel).  With DENSE_CLS_FOLD
# they are computed by workgroups at the end of the main launch's grid, on the CUs the dead tiles free (include/octic_hip.h:
# octic_dense_gemm_nt_tokens_adaptive_cls); same bits.  Effective only while DENSE_NARROW_DROPPED is on.  Read once at import from
# OCTIC_DENSE_CLS_FOLD (0 = off).
DENSE_CLS_FOLD = _skip_from_env("OCTIC_DENSE_CLS_FOLD")
# Smallest drop probability of the branch at which a launch asks for the fold.  The host cannot know the kept count without a
# sync, only its distribution: with 64 samples, 64 or more CUs are free while at most 38 are kept (5 x 38 = 190 narrow tiles), and
# when fewer are free the class-token workgroups run BEHIND the live tiles, where a K = 5120 item in one workgroup is slower
# than the two stand-alone launches.  The standalone table (NOTES.md, "class-token rows ride in the main launch") has the five
# launches of a block 61 / 54 us ahead with the fold at 32 / 38 kept, 37 us behind at 45 (31 CUs free for 80 workgroups), 42 ahead at
# 52 (the wide tile: 48 CUs free) and 60 behind at 64.  Kept is Binomial(64, 1 - drop): at drop 0.5, 0.95 of the draws are at most
# 38; at 0.4 half of them are and 0.06 are 45 or more; at 0.3 the mean is 45.
DENSE_CLS_FOLD_MIN_DROP = 0.4


def dense_cls_fold(drop_prob):
    """fold_cls of ops.dense_gemm_nt for a launch under the mask of a branch with this drop probability (None / 0: no draw)."""
    return bool(DENSE_CLS_FOLD and DENSE_NARROW_DROPPED and drop_prob is not None and float(drop_prob) >= DENSE_CLS_FOLD_MIN_DROP)


# The three multi-round launches of a block (qkv, fc1 + factor, fc2's input gradient) run on classic panels of 256 consecutive
# rows, which straddle two 257-token images and die only when both are dropped.  With DENSE_IMAGE_DROPPED a launch whose caller
# knows the branch's drop probability asks the library whether per-image panels - dead with their own image, class-token rows
# computed at the end of the same launch - are expected to be shorter (include/octic_hip.h: octic_dense_gemm_nt_tokens_image).
# Kept rows have the bits of the unmasked per-image launch.  The library moves qkv and fc2's input gradient; fc1 stays classic by
# its keep table (NOTES.md "Masked wide dense GEMMs").  Effective only while DENSE_NT_SKIP_DROPPED is on.  Read once at
# import from OCTIC_DENSE_IMAGE_SKIP (0 = off: the calls are exactly the former ones).
DENSE_IMAGE_DROPPED = _skip_from_env("OCTIC_DENSE_IMAGE_SKIP")


def dense_skip_scale(rs, rps, M, rows_to=None):
    """rs as the sample_scale of a dense_nt_kernel launch over M token rows: whole_sample_mask while the switch is on."""
    return whole_sample_mask(rs, rps, M, rows_to) if DENSE_NT_SKIP_DROPPED else None


# In the octic MLP the same factor makes the D8-GELU's work on a dropped sample void in both directions: gelu(h) of such a
# sample is read only by fc2 (whose fused tail multiplies the row by rs = 0) and by fc2's weight gradient (against zero dY rows),
# dh only by fc1's input and weight gradients, whose results for that sample are zero as well.  With LINEAR_SKIP_DROPPED the
# factor travels to the GELU kernels, which then move no input bytes for those rows and store zeros (zeros, not nothing: the
# readers multiply by 0, which is harmless on finite values only) - same launch shapes, same results.
# Read once at import from OCTIC_LINEAR_SKIP (0 = off).
LINEAR_SKIP_DROPPED = _skip_from_env("OCTIC_LINEAR_SKIP")


def linear_skip_scale(rs, rps, M, rows_to=None):
    """rs as the sample_scale of the octic MLP's row kernels over M token rows: whole_sample_mask while the switch is on."""
    return whole_sample_mask(rs, rps, M, rows_to) if LINEAR_SKIP_DROPPED else None


# The long-K GEMMs of an octic block (fc2 with its residual tail, the input gradients of fc1 and qkv) run the ring kernel, which
# writes every row: for them the factor travels as the `dropped` mask of octic_linear_d8_fwd_dropped - a promise about the INPUT (zero
# rows, or rs itself in a fused tail) instead of one about the output's readers.  The kernel then runs its live 128-row tiles
# first, dealt evenly over the XCDs, and writes zeros / the residual for the dead ones without loading them.  A switch of its
# own, effective only while LINEAR_SKIP_DROPPED is on: OCTIC_RING_SKIP (0 = off), read once at import.
RING_SKIP_DROPPED = _skip_from_env("OCTIC_RING_SKIP")


# The four weight gradients of an octic block (wgrad_ring_kernel, csrc/wgrad.hip) reduce over every token row, and every dY row
# of a dropped sample is an exact zero (proj and fc2: g = rs * dy; fc1: the D8-GELU backward of a zero cotangent; qkv: the
# attention backward of dO = 0).  With LINEAR_WGRAD_SKIP_DROPPED the factor travels to the kernel, which reads only the 32-row
# steps that touch a kept sample and deals them evenly over its row splits (include/octic_hip.h: octic_linear_d8_wgrad_skip) -
# same launch shapes, the f32 partial sums regrouped: same terms, last-bit differences.  The mask asks NO other switch (the
# layers hand it on by structure alone, d8_layers.py), so every bitwise on / off comparison of another switch sums alike in both
# arms.  Read once at import from OCTIC_LINEAR_WGRAD_SKIP (0 = off: the launches are exactly the former ones).
LINEAR_WGRAD_SKIP_DROPPED = _skip_from_env("OCTIC_LINEAR_WGRAD_SKIP")


def linear_wgrad_skip_scale(rs, rps, M):
    """rs as the sample_scale of a LinearD8 weight gradient over M token rows: whole_sample_mask while the switch is on."""
    return whole_sample_mask(rs, rps, M) if LINEAR_WGRAD_SKIP_DROPPED else None


def ring_skip_scale(rs, rps, M):
    """rs as the `dropped` mask of a ring-routed LinearD8 launch over M token rows: linear_skip_scale's conditions plus the
    switch above; None otherwise."""
    return linear_skip_scale(rs, rps, M) if RING_SKIP_DROPPED else None


# The LayerNorm that opens a branch receives its cotangent from the branch's first GEMM (qkv or fc1), whose input gradient is
# exactly zero in the rows of a sample the branch drops: LN'(0) = 0, so the norm's backward row pass needs neither those rows
# of the cotangent nor the stream rows and statistics that belong to them, and the rows add nothing to the norm's parameter
# gradients.  The same zeros make up half of what the qkv bias gradient sums.  With ROW_SKIP_DROPPED the factor travels to
# the backward row kernels (include/octic_hip.h: octic_dense_layernorm_bwd_tail_skip, octic_layernorm_d8_bwd*_skip,
# octic_dense_colsum_skip) - same launch shapes, same values.  Read once at import from OCTIC_ROW_SKIP (0 = off).
ROW_SKIP_DROPPED = _skip_from_env("OCTIC_ROW_SKIP")


def row_skip_scale(rs, rps, M, rows_to=None):
    """rs as the sample_scale of a backward row kernel over M token rows: whole_sample_mask while the switch is on."""
    return whole_sample_mask(rs, rps, M, rows_to) if ROW_SKIP_DROPPED else None


class RowSkipSlot:
    """One-slot holder through which the first GEMM of a branch hands the branch's stochastic-depth factor BACK to the node
    that produced its normalised input: that node runs before the factor is drawn, its backward after the consumer's forward.
    The producer keeps the slot on its ctx and attaches it to the normalised tensor (`_octic_row_skip`); a consumer that knows
    its input gradient is exactly zero in the rows of a dropped sample fills it in its forward (row_skip_fill); the
    producer's backward reads it (get).  Empty - nobody called row_skip_fill, a second call, another row count - means no
    mask.  What the slot cannot see is a reader that does NOT call row_skip_fill beside one that does (a plain torch op or
    user code on the same normalised tensor): its cotangent rows would be added to the promised zeros and dropped.  The
    guarantee is therefore for the paths of this package, where the normalised tensor goes to exactly one node (qkv or fc1,
    also through `_octic_prenorm` / `_prenorm`); code that hands it to anything else sets OCTIC_ROW_SKIP=0."""
    __slots__ = ("scale", "rps", "rows", "fills")

    def __init__(self):
        self.scale, self.rps, self.rows, self.fills = None, 0, 0, 0

    def get(self, rows):
        if self.fills != 1 or self.scale is None or self.rows != rows:
            return None, 0
        return self.scale, self.rps


def row_skip_attach(ctx, yn):
    """Producer side: a fresh slot on ctx and on the normalised tensor."""
    ctx.row_skip = yn._octic_row_skip = RowSkipSlot()


def row_skip_fill(x, scale, rps, rows):
    """Consumer side: x is the tensor the node was handed; scale = row_skip_scale(...) of the branch (None voids nothing: an
    unfilled slot already means no mask, but the visit counts - two readers of one normalised tensor sum their cotangents)."""
    slot = getattr(x, "_octic_row_skip", None)
    if slot is not None:
        slot.fills += 1
        slot.scale, slot.rps, slot.rows = scale, rps, rows


def row_skip_get(ctx, rows):
    slot = getattr(ctx, "row_skip", None)
    return (None, 0) if slot is None else slot.get(rows)


# What the masked backward row kernels still move for the rows of a dropped sample is a copy: dx = dres, read from the incoming
# stream cotangent and written to a fresh tensor.  With ROW_INPLACE the two are one buffer (include/octic_hip.h:
# octic_dense_layernorm_bwd_tail_inplace, octic_layernorm_d8_bwd_cast_inplace): live rows are updated in place, dead rows are
# not written, and not read either where the branch that ended in front of the norm dropped the sample too.  The same switch
# routes the forward tail to octic_dense_resid_layernorm_fwd_skip (yb unread where rs is 0).  Effective only while
# ROW_SKIP_DROPPED is on; read once at import from OCTIC_ROW_INPLACE (0 = off).
ROW_INPLACE = _skip_from_env("OCTIC_ROW_INPLACE")


class OwnedStreamGrad:
    """Which stream cotangent may be written into: only a buffer that a backward node of this package allocated itself and
    handed to autograd as the cotangent of its stream input, in the backward pass that is still running.  The node that returns
    it calls offer(); the node that receives a stream cotangent calls take(), which is True for exactly that buffer (same
    pass, same address, size, dtype and storage) and consumes the entry.  A tensor the caller passed to `.backward(g)`, a sum
    autograd formed of two cotangents, a cast or a copy is never offered and so never written.  One entry: the stream is a
    chain, each cotangent has one consumer.  The storage is held until the entry is replaced or the pass ends, so the address
    cannot be handed to somebody else in between.  The limit: a `retain_grad()` or a tensor hook on a stream tensor INSIDE the
    package's path keeps a reference to the offered buffer and sees it updated in place; such code sets OCTIC_ROW_INPLACE=0."""
    __slots__ = ("task", "ptr", "numel", "storage", "armed")

    def __init__(self):
        self.task, self.ptr, self.numel, self.storage, self.armed = -1, 0, 0, None, -1

    def clear(self):
        self.task, self.ptr, self.numel, self.storage = -1, 0, 0, None

    def offer(self, dx):
        if dx is None or not (ROW_INPLACE and ROW_SKIP_DROPPED and ops._in_backward()):
            return
        task = torch._C._current_graph_task_id()
        self.task, self.ptr, self.numel, self.storage = task, dx.data_ptr(), dx.numel(), dx.untyped_storage()
        if self.armed != task:
            self.armed = task
            torch.autograd.Variable._execution_engine.queue_callback(self.clear)

    def take(self, g):
        st, ptr, numel, task = self.storage, self.ptr, self.numel, self.task
        if st is None:
            return False
        self.clear()
        return (ROW_INPLACE and ROW_SKIP_DROPPED and ops._in_backward() and task == torch._C._current_graph_task_id()
                and g.dtype == torch.float32 and g.is_contiguous() and g.data_ptr() == ptr and g.numel() == numel
                and g.untyped_storage().data_ptr() == st.data_ptr())


STREAM_GRADS = OwnedStreamGrad()


class AttnPackedFn(torch.autograd.Function):
    """AttentionD8's core on packed rows (reference d8_layers.py:631-656): qkv [B,T,3*8c] -> o [B,T,8c].  The head
    vectors are gathered from / scattered to the irrep pieces inside the attention kernels, so the four pack / unpack
    passes of a training step (and their 0.5 GB of traffic per block) do not exist."""

    @staticmethod
    def forward(ctx, qkv, H, c, scale, sample_scale=None):
        qkv = _c(qkv)
        ss = skip_scale(sample_scale, qkv.shape[0])
        o, lse = ops.attn_fwd_packed(qkv, H, c, scale, sample_scale=ss)
        ctx.save_for_backward(qkv, o, lse, ss)
        ctx.meta = (H, c, scale)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, ss = ctx.saved_tensors
        H, c, scale = ctx.meta
        return ops.attn_bwd_packed(qkv, o, _c(do), lse, H, c, scale, sample_scale=ss), None, None, None, None


class AttnFusedQKVFn(torch.autograd.Function):
    """Attention on a fused projection output qkv [B,T,3,H,hd] (the layout of the standard block, deit/vit.py:38-39):
    q/k/v are read through strides, the result is written as [B,T,H*hd] and the gradient comes back as ONE
    [B,T,3,H,hd] tensor (no permute copies, no zero-fill + add of three partial gradients)."""

    @staticmethod
    def forward(ctx, qkv, scale, sample_scale=None):
        qkv = _c(qkv)
        B, T, _, H, hd = qkv.shape
        ss = skip_scale(sample_scale, B) if qkv.dtype == torch.bfloat16 else None
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.empty((B, T, H, hd), dtype=qkv.dtype, device=qkv.device)
        ov = o.permute(0, 2, 1, 3)
        _, lse = ops.attn_fwd(q, k, v, scale, out=ov, sample_scale=ss)     # bf16 or float32 entry point by qkv.dtype
        ctx.save_for_backward(qkv, o, lse, ss)
        ctx.scale = scale
        return o.view(B, T, H * hd)

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse, ss = ctx.saved_tensors
        B, T, _, H, hd = qkv.shape
        do = _c(do).view(B, T, H, hd)
        dqkv = torch.empty_like(qkv)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        ops.attn_bwd(q, k, v, o.permute(0, 2, 1, 3), do.permute(0, 2, 1, 3), lse, ctx.scale, dq, dk, dv, sample_scale=ss)
        return dqkv, None, None


def attention_core(q, k, v, dropout_p=0.0):
    """Drop-in for F.scaled_dot_product_attention(q, k, v) on [B,H,T,hd]: HIP kernels for the shapes they cover (bf16 and
    float32 operands, T <= 16384, head_dim a multiple of 16 up to 128, no dropout); torch SDPA only for attention dropout
    > 0, fp16 tensors, head sizes that are not multiples of 16 and CPU tensors."""
    B, H, T, hd = q.shape
    if dropout_p == 0.0 and q.is_cuda and (ops.attn_supported(T, hd, q.dtype) or ops.attn_f32_supported(T, hd, q.dtype)):
        return AttnFn.apply(q, k, v, hd ** -0.5)
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p)
    return o if o.dtype == q.dtype else o.to(q.dtype)       # fp16 autocast hands back fp16: the octic rows stay in q's dtype


# -------------------------------------------------------------------------------------- standard half
class DenseWeightCache:
    """Compute-dtype copy of an nn.Linear's weight and bias, refreshed when the master parameters change."""

    def __init__(self):
        self.key = None
        self.w = self.b = None
        self.wt = self.wt_key = None
        self.static = False         # the copies are refreshed IN PLACE by their producer after every optimizer step (adopt):
        self.static_wt = False      # a traced graph may read them as plain inputs (dispatch.py)

    def static_nt(self):
        """(bf16 W, bf16 W^T or None) when the fused optimizer keeps them current in place, else (None, None)."""
        # (reads nothing that changes from step to step - no keys, no version counters: torch.compile guards on what a traced
        # function reads, and a guard on a version counter would recompile the block after every optimizer step)
        if self.static and self.w is not None and self.w.dtype == torch.bfloat16:
            return self.w, (self.wt if self.static_wt else None)
        return None, None

    @staticmethod
    def _key(w, b, dtype):
        return (dtype, w.data_ptr(), w._version, None if b is None else (b.data_ptr(), b._version))

    def get(self, w, b, dtype):
        key = self._key(w, b, dtype)
        if key != self.key:
            with torch.no_grad():
                self.w = _c(w.detach().to(dtype))
                self.b = None if b is None else _c(b.detach().to(dtype))
            self.key = key
            self.wt, self.wt_key = None, None     # a transposed copy of the old cast is stale with it
            self.static = self.static_wt = False
        return self.w, self.b

    def adopt(self, w, b, w_copy, b_copy, dtype, wt_copy=None):
        """Take compute-dtype copies produced elsewhere (the fused optimizer writes them in its update pass) as the
        current cache content for the parameters' present versions."""
        self.w, self.b = w_copy, b_copy
        self.key = self._key(w, b, dtype)
        self.static = True
        self.static_wt = wt_copy is not None
        if wt_copy is not None:
            self.wt, self.wt_key = wt_copy, self.key

    def get_nt(self, w, b, need_wt=True):
        """(bf16 W [N,K], bf16 W^T [K,N] or None) for the hand-written dense GEMMs (forward / input-gradient operands);
        the transposed copy only exists for layers whose input gradient runs on csrc/dense_gemm.hip."""
        wb, _ = self.get(w, b, torch.bfloat16)
        if not need_wt:
            return wb, None
        if self.wt is None or self.wt_key != self.key:
            with torch.no_grad():
                self.wt = wb.t().contiguous()
            self.wt_key = self.key
        return wb, self.wt


class SoftCrossEntropyFn(torch.autograd.Function):
    """Per row of the student logits s [N, K]: -sum_k t_k log_softmax(s / temp)_k against the teacher probabilities
    tprob [Nt, K] (f32, no gradient; row r uses tprob[r % Nt]) -> [N] f32.  One read of s and tprob forward, one read of each
    and one write backward (csrc/ssl_loss.hip) - dinov2/loss/dino_clstoken_loss.py:78-92, ibot_patch_loss.py:26-34."""

    @staticmethod
    def forward(ctx, s, tprob, temp):
        tprob = _c(tprob.detach().float())
        loss, lse, tsum = ops.soft_ce_fwd(s, tprob, 1.0 / temp)
        ctx.save_for_backward(s, tprob, lse, tsum)
        ctx.temp = temp
        return loss

    @staticmethod
    def backward(ctx, g):
        s, tprob, lse, tsum = ctx.saved_tensors
        return ops.soft_ce_bwd(s, tprob, 1.0 / ctx.temp, g, lse, tsum), None, None


def loss_rows_ok(t):
    """The prototype-axis row kernels take this tensor (GPU, f32 / bf16, rows of K % 8 == 0 elements)."""
    return t.is_cuda and t.dtype in (torch.float32, torch.bfloat16) and t.shape[-1] % 8 == 0 and not torch.compiler.is_compiling()


class KoLeoFn(torch.autograd.Function):
    """KoLeo terms of x [groups * n, D] (f32 / bf16), read as `groups` independent groups of n consecutive rows -> [groups * n]
    f32, term_i = -log(||xh_i - xh_nn(i) + 1e-8|| + eps) with xh the rows normalised with F.normalize's eps and nn(i) the nearest
    other row of the group (largest dot, lowest index on ties).  One launch forward, one backward (csrc/koleo.hip) -
    dinov2/loss/koleo_loss.py:25-48; the loss of a group is the mean of its terms."""

    @staticmethod
    def forward(ctx, x, groups, eps=1e-8):
        term, nn, inv, dist = ops.koleo_fwd(x, groups, eps)
        ctx.save_for_backward(x, nn, inv, dist)
        ctx.groups, ctx.eps = groups, eps
        return term

    @staticmethod
    def backward(ctx, g):
        x, nn, inv, dist = ctx.saved_tensors
        return ops.koleo_bwd(x, ctx.groups, g, nn, inv, dist, ctx.eps).view(x.shape), None, None


def koleo_rows_ok(x, groups):
    """x takes the KoLeo kernels as `groups` groups of consecutive rows: a 2-D GPU tensor, f32 / bf16, unit column stride, not
    under torch.compile tracing, and a shape octic_koleo_ok admits."""
    return bool(x.dim() == 2 and x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1
                and not torch.compiler.is_compiling() and groups >= 1 and x.shape[0] % groups == 0
                and ops.koleo_ok(groups, x.shape[0] // groups, x.shape[1]))


class DenseLayerNormFn(torch.autograd.Function):
    """nn.LayerNorm over the last dim of an f32 residual stream, result in the compute dtype.  Returns (y, x): the
    second output is the stream itself, to be used for the residual connection, so that the residual cotangent
    comes back through this node and is added inside the backward kernel instead of by a separate pass."""

    @staticmethod
    def forward(ctx, x, w, b, eps, out_dtype):
        x = _c(x)
        w32 = None if w is None else _c(w.detach().float())
        b32 = None if b is None else _c(b.detach().float())
        y, stats = ops.dense_layernorm_fwd(x, w32, b32, eps, out_dtype)
        ctx.save_for_backward(x, stats, w32)
        ctx.has_w, ctx.has_b = w is not None, b is not None
        ctx.set_materialize_grads(False)
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gres):
        x, stats, w32 = ctx.saved_tensors
        if gy is None:
            return gres, None, None, None, None
        want = ctx.has_w and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dres = None if gres is None else _c(gres.float())
        dx, dw, db = ops.dense_layernorm_bwd(_c(gy), x, w32, stats, dres, want_param_grads=want)
        return dx, (dw if ctx.has_w else None), (db if ctx.has_b else None), None, None


class RowsTo:
    """Where the tail of a branch that saw only some rows of the residual stream puts its result: rows `rowmap[r]` of
    `stream` (int32 map, one entry per compact row), in place.  `link` carries the stream's cotangent from the tail's backward
    to the LayerNorm's (DenseLayerNormRowsFn), which edits it in place - DINOv2's batch-subset stochastic depth
    (dinov2/layers/block.py:113-140) without gather / scatter passes."""
    __slots__ = ("stream", "rowmap", "link")

    def __init__(self, stream, rowmap, link):
        self.stream, self.rowmap, self.link = stream, rowmap, link


class _Link:
    __slots__ = ("g",)

    def __init__(self):
        self.g = None


class DenseLayerNormRowsFn(torch.autograd.Function):
    """LayerNorm of rows rowmap[r] of the f32 stream -> (y compute dtype, xa f32): both compact [1, rows, d]; xa = the rows as
    read (the residual input of the branch's tail, and what the backward needs after the stream was edited in place).
    Backward: the stream's cotangent g arrives through `link` (set by the tail's backward, which returns no gradient for xa);
    g[rowmap[r]] = LN'(gy[r]) + g[rowmap[r]] in place, and g is returned as the gradient of the stream."""

    @staticmethod
    def forward(ctx, stream, rowmap, w, b, eps, out_dtype, link):
        if stream.dtype != torch.float32 or not stream.is_contiguous():
            raise ValueError("DenseLayerNormRowsFn: the stream must be a contiguous f32 tensor (it is edited in place)")
        w32 = None if w is None else _c(w.detach().float())
        b32 = None if b is None else _c(b.detach().float())
        y, stats, xa = ops.dense_layernorm_fwd_rows(stream, rowmap, w32, b32, eps, out_dtype)
        ctx.save_for_backward(xa, stats, w32, rowmap)
        ctx.has_w, ctx.has_b, ctx.link = w is not None, b is not None, link
        ctx.set_materialize_grads(False)
        return y, xa

    @staticmethod
    def backward(ctx, gy, gxa):
        xa, stats, w32, rowmap = ctx.saved_tensors
        g, ctx.link.g = ctx.link.g, None
        if g is None or gxa is not None or gy is None:
            raise RuntimeError("DenseLayerNormRowsFn: expects the stream cotangent through its link (RowsTo tail) and no direct "
                               "gradient for the compact rows")
        want = ctx.has_w and (ctx.needs_input_grad[2] or ctx.needs_input_grad[3])
        dw, db = ops.dense_layernorm_bwd_rows_(_c(gy), xa, w32, stats, g, rowmap, want_param_grads=want)
        return g, None, (dw if ctx.has_w else None), (db if ctx.has_b else None), None, None, None


class DenseLinearFn(torch.autograd.Function):
    """nn.Linear with cached compute-dtype weights (no per-step cast kernels in the graph): float32 on the GPU runs on
    csrc/dense_f32.hip (DENSE_F32_HIP), everything else on the BLAS library."""

    @staticmethod
    def forward(ctx, x, w, b, dtype, cache):
        ops._require_cuda(x)
        xb = _c(x if x.dtype == dtype else x.to(dtype))
        wb, bb = cache.get(w, b, dtype)
        x2 = xb.reshape(-1, wb.shape[1])
        ctx.f32 = dense_f32_hip_ok(x2.shape[0], wb.shape[0], wb.shape[1], x2, wb)
        if ctx.f32:
            y = ops.dense_f32_nt(x2, wb, bb).view(*xb.shape[:-1], wb.shape[0])
        else:
            with torch.autocast("cuda", enabled=False):
                y = torch.nn.functional.linear(xb, wb, bb)
        ctx.save_for_backward(xb, wb)
        ctx.has_b, ctx.x_dtype = b is not None, x.dtype
        ctx.wparam = w
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, wb = ctx.saved_tensors
        g2, x2 = _c(gy).reshape(-1, wb.shape[0]), xb.reshape(-1, wb.shape[1])
        if ctx.f32:
            gx = ops.dense_f32_nn(g2, wb).view(xb.shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            gw, gb = _wgrad_f32(g2, x2, ctx.wparam, want_colsum=ctx.has_b)
            return gx, gw, gb, None, None
        with torch.autocast("cuda", enabled=False):
            gx = (g2 @ wb).view(xb.shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            gw = (g2.t() @ x2).float()
            gb = g2.sum(0, dtype=torch.float32) if ctx.has_b else None
        return gx, gw, gb, None, None


class DenseLinearGeluFn(torch.autograd.Function):
    """gelu(x W^T + b) of the standard MLP.  bf16: library GEMM with bias epilogue + torch's exact GELU forward; the
    backward is one HIP pass that yields dh = gelu'(h) g and the bias gradient (column sums of dh) together.  float32
    (dtype = torch.float32, shapes dense_f32_hip_ok takes): the GEMM of csrc/dense_f32.hip with the GELU in its epilogue, h
    saved, the backward through ops.dense_gelu_bwd_f32 and the float32 NN / TN kernels."""

    @staticmethod
    def forward(ctx, x, w, b, cache, dtype=torch.bfloat16):
        ops._require_cuda(x)
        xb = _c(x if x.dtype == dtype else x.to(dtype))
        wb, bb = cache.get(w, b, dtype)
        ctx.f32 = dtype == torch.float32
        if ctx.f32:
            x2 = xb.reshape(-1, wb.shape[1])
            if not dense_f32_hip_ok(x2.shape[0], wb.shape[0], wb.shape[1], x2, wb):
                raise RuntimeError("DenseLinearGeluFn: float32 needs the dense_f32 kernels (check dense_f32_hip_ok first)")
            h, y = ops.dense_f32_nt(x2, wb, bb, gelu=True)
            h, y = h.view(*xb.shape[:-1], wb.shape[0]), y.view(*xb.shape[:-1], wb.shape[0])
        else:
            with torch.autocast("cuda", enabled=False):
                h = torch.nn.functional.linear(xb, wb, bb)
                y = torch.nn.functional.gelu(h)
        ctx.save_for_backward(xb, wb, h)
        ctx.has_b, ctx.x_dtype = b is not None, x.dtype
        ctx.wparam = w
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, wb, h = ctx.saved_tensors
        if ctx.f32:
            dh, db = ops.dense_gelu_bwd_f32(h, _c(gy.to(h.dtype)), want_colsum=ctx.has_b)
            g2, x2 = dh.reshape(-1, wb.shape[0]), xb.reshape(-1, wb.shape[1])
            gx = ops.dense_f32_nn(g2, wb).view(xb.shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            return gx, _wgrad_f32(g2, x2, ctx.wparam)[0], db, None, None
        dh, db = ops.dense_gelu_bwd(h, _c(gy.to(h.dtype)), want_colsum=ctx.has_b)
        g2, x2 = dh.reshape(-1, wb.shape[0]), xb.reshape(-1, wb.shape[1])
        with torch.autocast("cuda", enabled=False):
            gx = (g2 @ wb).view(xb.shape).to(ctx.x_dtype) if ctx.needs_input_grad[0] else None
            gw = (g2.t() @ x2).float()
        return gx, gw, db, None, None


class LinearScaleResidualFn(torch.autograd.Function):
    """Tail of a standard block branch:  out = x + rs * gamma * (a W^T + b)  with x the f32 residual stream, a the
    compute-dtype branch activations, gamma the layer scale [d] and rs the per-sample stochastic-depth factor
    (both optional).  The GEMMs are the library's (float32: those of csrc/dense_f32.hip, through _linear_lib / _mm_lib /
    _wgrad_lib); everything around them is one HIP pass each way, which also yields d gamma and the bias gradient."""

    @staticmethod
    def forward(ctx, x, a, w, b, gamma, rs, rps, dtype, cache):
        ops._require_cuda(x)
        x = _c(x)
        ab = _c(a if a.dtype == dtype else a.to(dtype))
        wb, bb = cache.get(w, b, dtype)
        y = _linear_lib(ab.reshape(-1, wb.shape[1]), wb, bb).view(*ab.shape[:-1], wb.shape[0])
        g32 = None if gamma is None else _c(gamma.detach().float())
        rs32 = None if rs is None else _c(rs.detach().float())
        out = ops.scale_residual_fwd(x, y, g32, rs32, rps)
        ctx.save_for_backward(ab, wb, y, g32, rs32)
        ctx.meta = (rps, b is not None, gamma is not None, a.dtype)
        ctx.wparam = w
        return out

    @staticmethod
    def backward(ctx, gout):
        ab, wb, y, g32, rs32 = ctx.saved_tensors
        rps, has_b, has_gamma, a_dtype = ctx.meta
        gout = _c(gout.float())
        gy, dgamma, colsum = ops.scale_residual_bwd(gout, y, g32, rs32, rps, want_gamma=has_gamma, want_colsum=has_b)
        g2, a2 = gy.reshape(-1, wb.shape[0]), ab.reshape(-1, wb.shape[1])
        ga = _mm_lib(g2, wb).view(ab.shape).to(a_dtype) if ctx.needs_input_grad[1] else None
        gw = _wgrad_lib(g2, a2, ctx.wparam)
        return gout, ga, gw, colsum, dgamma, None, None, None, None


def invalidate_weight_caches(model):
    """Drop every cached compute-dtype weight copy below ``model`` (LinearD8 ``WeightPrep``s, the standard half's
    ``DenseWeightCache``s): the next forward re-casts from the master parameters.

    The caches key on ``(data_ptr, tensor._version)``.  An optimizer that writes through ``p.data`` or raw pointers
    (apex FusedLAMB — the reference recipe's optimizer — updates ``p.data`` in a multi-tensor kernel) does not bump
    ``_version``, so such optimizers MUST call this after every step; ``track_optimizer`` installs it as a
    step post-hook.  The repo's own ``FusedLamb`` advances the version counters itself."""
    n = 0
    for m in model.modules():
        for attr in ("_prep", "_c1", "_c2"):
            c = getattr(m, attr, None)
            if isinstance(c, (WeightPrep, DenseWeightCache)):
                c.key = None
                if isinstance(c, DenseWeightCache):
                    # the transposed copy (operand of the hand-written input-gradient GEMM) keys on `key`; a re-cast
                    # restores the same key (data_ptr and _version are unchanged by a raw write), so drop it explicitly
                    c.wt, c.wt_key = None, None
                n += 1
    return n


def track_optimizer(model, optimizer):
    """Register ``invalidate_weight_caches(model)`` as a post-step hook of a torch.optim.Optimizer (any optimizer,
    including ones that update ``p.data`` behind autograd's back).  Returns the hook handle."""
    return optimizer.register_step_post_hook(lambda *_a, **_k: invalidate_weight_caches(model))


# --------------------------------------------------------------- standard half on the hand-written MFMA GEMMs
# Which GEMMs of a standard block run on csrc/dense_gemm.hip (the others would go to the BLAS library + the row kernels
# of csrc/dense.hip).  Measured in the train step on MI355X (same device, back to back; DESIGN.md section 3.5;
# tools/ab_dense.sh): since round 3 (tail tiles in front of the grid, rows past M never travel, no split where the slab
# round trip costs more than the K loop it saves, fc1's bias gradient out of the GELU' epilogue) all eight on the
# hand-written kernel is level with or ahead of every mixed routing (72.2 vs 72.3-72.9 ms per step), so the whole
# standard half is hand-written; per shape the library is still ahead on proj (N = K = 1280: 62 vs 67 us, two rounds of
# 256 x 256 tiles against its 256 x 192 ones) and that is paid back by the fused tails (no scale_residual_fwd, no
# dense_gelu_bwd pass).
WGRAD_F32_OUT = False      # True: library weight gradients as torch.mm(..., out_dtype=float32) (no bf16 rounding of
                           # dW; measured equal in step time, but outside the shipped TunableOp table)
DENSE_HIP = {"qkv", "dqkv", "proj", "dproj", "fc1", "dfc1", "fc2", "dfc2"}    # any subset (bench.py --dense-hip)
# proj / fc2 on the hand-written kernel: x + rs*gamma*y inside the GEMM's epilogue (True) or as the separate row kernel
# after a plain epilogue (False).  The fused tail reads and writes the f32 residual stream tile by tile at the end of a
# workgroup with nothing to overlap it (one workgroup per CU): in the step it costs more than the 35 us row pass.
DENSE_RESID_FUSED = False
# The residual add of a branch and the LayerNorm that opens the next one (norm2 of the same block, norm1 of the next
# block) as ONE row pass (csrc/dense.hip dense_resid_ln_fwd_kernel): the f32 stream is written once and not read back.
NEXT_NORM_FUSED = True
# Octic half: the residual-fused proj / fc2 and the LayerNormD8 that follows as one autograd node (LinearD8NormFn): the
# norm's backward also emits the drop-path-scaled bf16 cotangent of the branch (no cast_rowscale pass).
OCTIC_NEXT_NORM = True
# ... and in the backward of that pair: LayerNorm backward + the backward of the residual tail in front of it as one row
# pass (dense_ln_bwd_tail_kernel) instead of dense_ln_bwd + scale_residual_bwd (the stream cotangent is not read back).
LN_TAIL_FUSED = True


def dense_hip_ok(x, w, which=None):
    """bf16 autocast on the GPU, a shape csrc/dense_gemm.hip covers in BOTH directions (forward: K = in_features,
    input gradient: K = out_features; the kernel needs K % 64 == 0, K >= 128, N % 8 == 0) and routed."""
    rows = x.numel() // max(1, x.shape[-1])
    return (which is None or which in DENSE_HIP) and x.is_cuda and ops.dense_gemm_ok(rows, w.shape[0], w.shape[1])


def _f32(t):
    return None if t is None else _c(t.detach().float())


def _timed_lib(kind, fn, M, N, K):
    """Run a BLAS-library GEMM under the kernel timer (bench.py's `kernels` / `roofline` cover the whole step, not only
    the engine's own launches): name = library_gemm<kind N x K>, 2 M N K flops, operand + result bytes."""
    t = ops.KERNEL_TIMER.start()
    out = fn()
    if t is not None:
        ops.KERNEL_TIMER.stop(t, f"library_gemm<{kind} {N}x{K}>", 2 * (M * K + N * K + M * N), 2.0 * M * N * K)
    return out


# Row slabs of the library weight gradients (the fallback path: shapes csrc/dense_wgrad.hip refuses, or WGRAD_HIP off).
# dW [N,K] = g^T x reduces over the token rows into few output tiles (100 tiles of 256x256 for 5120x1280: the single GEMM
# leaves more than a third of the 256 CUs idle and runs at 0.43-0.79 PFLOP/s).  As a batched GEMM over S row slabs the
# same library kernels fill the chip; the slab partials (bf16, like the single GEMM's result) are summed in f32 by one
# small reduction that replaces the bf16 -> f32 cast.  Measured on MI355X (tools/probe_wgrad_split.py): 311 -> 263,
# 284 -> 247, 217 -> 188, 124 -> 92 us.  WGRAD_SLABS holds the measured choices; other shapes take the rule
# "one round of 256 x 256 tiles over the CUs" (wgrad_slabs), False switches slabs off (bench.py --no-wgrad-slabs).
WGRAD_SLABS = {(5120, 1280): 4, (1280, 5120): 4, (3840, 1280): 2, (1280, 1280): 2}


def wgrad_slabs(M, N, K):
    if WGRAD_SLABS is False:
        return 1
    S = WGRAD_SLABS.get((N, K))
    if S is None:
        tiles = -(-N // 256) * -(-K // 256)
        S = max(1, min(8, 256 // max(1, tiles)))
    while S > 1 and M % S:
        S -= 1
    return S


# Weight gradients of the standard half on csrc/dense_wgrad.hip (dW = dY^T X straight from the row-major operands, f32
# result, fixed-order slab reduction) wherever the kernel takes the shape (ops.dense_wgrad_ok: the library's plan and
# a cap of 256 output tiles - ViT-H/14, ViT-L/16, ...), not for a literal list of shapes (round-3 review).  Measured against
# the library's batched row slabs on one MI355X (tools/bench_tn.py): 5120x1280 224-234 vs 296 us, 1280x5120 211 vs 246,
# 3840x1280 156 vs 187, 1280x1280 93 vs 100.  False = every weight gradient on the BLAS library (bench.py --lib-wgrad).
WGRAD_HIP = True

# The GEMMs of a float32 standard block (and the float32 calls of the seams below) on csrc/dense_f32.hip: exact-f32 MFMA,
# bitwise repeatable, a sample's rows independent of its batch mates.  False = today's BLAS-library calls, bit for bit.
DENSE_F32_HIP = True


def dense_f32_hip_ok(M, N, K, *operands):
    """A GEMM of a linear layer with M rows, N = out_features, K = in_features goes to csrc/dense_f32.hip: the switch is on,
    torch.compile is not tracing, every operand is a CUDA float32 2-D tensor with unit column stride, and the library takes
    the shape and the strides (ops.dense_f32_ok: one answer for the layer's three GEMMs)."""
    if not DENSE_F32_HIP or torch.compiler.is_compiling():
        return False
    if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 for t in operands):
        return False
    # (the results are dense: their row strides are N and K; a one-row operand's stride is whatever torch left there)
    return M >= 1 and ops.dense_f32_ok(M, N, K, max([N, K] + [t.stride(0) for t in operands if t.shape[0] > 1]))


def _wgrad_f32(g2, x2, wparam=None, want_colsum=False):
    """(dW [N,K], db [N] or None) = (g2^T x2, column sums of g2) on the float32 TN kernel, written into the parameter's
    registered gradient destination where there is one (ops.grad_dest)."""
    dest = ops.grad_dest(wparam, (g2.shape[1], x2.shape[1]))
    out = ops.dense_f32_tn(g2, x2, out=dest, want_colsum=want_colsum)
    if dest is not None:
        ops.grad_written(wparam)
    return out if want_colsum else (out, None)


def _wgrad_lib(g2, x2, wparam=None, sample_scale=None, rps=0):
    """dW = g^T x (f32 result): the hand-written TN kernel wherever it takes the shape, else the BLAS library.  wparam: the
    parameter this is the gradient of - under DDP the result is written into its bucket view (ops.GRAD_DEST).
    sample_scale / rps (wgrad_skip_scale): the stochastic-depth mask of g2's branch, for the hand-written kernel only."""
    M, N, K = g2.shape[0], g2.shape[1], x2.shape[1]
    if dense_f32_hip_ok(M, N, K, g2, x2):
        return _wgrad_f32(g2, x2, wparam)[0]
    if (WGRAD_HIP and g2.is_cuda and g2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16
            and g2.stride(1) == 1 and x2.stride(1) == 1
            and ops.dense_wgrad_ok(M, N, K, max(g2.stride(0), x2.stride(0)))):
        dest = ops.grad_dest(wparam, (N, K))
        dw = ops.dense_wgrad_tn(g2, x2, out=dest, sample_scale=sample_scale, rows_per_sample=rps)
        if dest is not None:
            ops.grad_written(wparam)
        return dw
    S = wgrad_slabs(M, N, K)
    if S > 1 and g2.is_contiguous() and x2.is_contiguous():
        with torch.autocast("cuda", enabled=False):
            return _timed_lib("wgrad", lambda: torch.bmm(g2.view(S, M // S, N).transpose(1, 2), x2.view(S, M // S, K))
                              .sum(0, dtype=torch.float32), M, N, K)
    with torch.autocast("cuda", enabled=False):
        if WGRAD_F32_OUT:
            # bf16 operands, f32 result straight from the GEMM: no bf16 rounding of the gradient, no cast launch
            return _timed_lib("wgrad", lambda: torch.mm(g2.t(), x2, out_dtype=torch.float32), g2.shape[0], g2.shape[1],
                              x2.shape[1])
        w = _timed_lib("wgrad", lambda: g2.t() @ x2, g2.shape[0], g2.shape[1], x2.shape[1])
        return w.float()


def _mm_lib(a2, b):
    """a2 [M,N] @ b [N,K]: the input-gradient GEMM of 2-D tensors - float32 on csrc/dense_f32.hip (dense_f32_hip_ok), anything
    else (bf16) on the library (no autocast re-casts)."""
    if dense_f32_hip_ok(a2.shape[0], b.shape[0], b.shape[-1], a2, b):
        return ops.dense_f32_nn(a2, b)
    with torch.autocast("cuda", enabled=False):
        return _timed_lib("dgrad", lambda: a2 @ b, a2.shape[0], b.shape[1], b.shape[0])


def _linear_lib(x2, wb, bias):
    """x2 [M,K] @ wb [N,K]^T + bias: float32 on csrc/dense_f32.hip (dense_f32_hip_ok), anything else on the library."""
    if dense_f32_hip_ok(x2.shape[0], wb.shape[0], wb.shape[-1], x2, wb) and (bias is None or bias.dtype == torch.float32):
        return ops.dense_f32_nt(x2, wb, None if bias is None else _c(bias))
    with torch.autocast("cuda", enabled=False):
        return _timed_lib("fwd", lambda: torch.nn.functional.linear(x2, wb, bias), x2.shape[0], wb.shape[0], wb.shape[1])


# The qkv and proj weight gradients of a standard block as ONE launch (ops.dense_wgrad_tn_pair): proj's backward runs first and
# parks its operands in the Attention module's WgradPair; qkv's backward, one attention backward later, launches both.  The
# parked gradient tensor is handed to autograd UNWRITTEN in between - only where nothing can read it before the end of the
# backward pass, i.e. under the same condition as ops.DEFERRED_FINISHES (train.Trainer: one micro-batch into .grad = None, no
# DDP hooks); elsewhere both run at once as before.  1280 x 1280 alone is 25 tiles x 8 row slabs at 0.6 PFLOP/s (90 us); beside
# the 75 tiles of 3840 x 1280 the pair is a 100-tile, two-slab launch like the MLP weights.
WGRAD_PAIRED = True
GELU_FACTOR = True     # standard MLP: keep gelu'(h) instead of h between fc1's forward and fc2's input gradient (bench --no-gelu-factor)


class WgradPair:
    __slots__ = ("pending",)

    def __init__(self):
        self.pending = None

    def park(self, g2, x2, wparam=None, sample_scale=None, rps=0):
        """Postpone dW = g2^T x2; returns the (not yet written) result tensor - the registered destination of `wparam`'s
        gradient where there is one (ops.GRAD_DEST).  sample_scale / rps: g2's stochastic-depth mask (wgrad_skip_scale),
        kept with the operands for whichever launch runs them."""
        shape = (g2.shape[1], x2.shape[1])
        dw = ops.grad_dest(wparam, shape)
        landed = wparam if dw is not None else None
        if dw is None:
            dw = torch.empty(shape, dtype=torch.float32, device=g2.device)
        # (storage, not tensor: a second tensor reference would make AccumulateGrad clone the unwritten gradient)
        self.pending = (g2, x2, dw.untyped_storage(), dw.data_ptr(), tuple(dw.shape), dw.storage_offset(), landed,
                        sample_scale, rps)
        ops.DEFERRED_FINISHES.add_pair(self)
        return dw

    def take(self):
        """(g2, x2, dw, landed, sample_scale, rps): landed = the parameter whose registered gradient destination dw is, or
        None; sample_scale / rps = the mask park() was given."""
        p, self.pending = self.pending, None
        if p is None:
            return None
        g2, x2, storage, ptr, shape, offset, landed, ss, rps = p
        dw = torch.empty(0, dtype=torch.float32, device=g2.device).set_(storage, offset, shape)
        assert dw.data_ptr() == ptr
        return g2, x2, dw, landed, ss, rps

    def flush(self):
        p = self.take()
        if p is not None:
            g2, x2, dw, landed, ss, rps = p
            dw.copy_(_wgrad_lib(g2, x2, sample_scale=ss, rps=rps))
            ops.grad_written(landed)


def _pair_ready(pair, g2, x2):
    return (pair is not None and WGRAD_PAIRED and WGRAD_HIP and ops.DEFERRED_FINISHES.enabled
            and ops.DEFERRED_FINISHES.allow_pairs and ops._in_backward()
            and g2.is_cuda and g2.dtype == torch.bfloat16 and x2.dtype == torch.bfloat16 and g2.stride(1) == 1
            and x2.stride(1) == 1)


def _tok(shape):
    """Tokens per image of a [B, tokens, C] activation (0 = not known to be whole images): lets csrc/dense_gemm.hip take
    per-image row panels for ViT-H/14's 257-token images (octic_dense_gemm_nt_tokens)."""
    return int(shape[-2]) if len(shape) >= 3 else 0


def _gemm_fwd(tag, x2, wb, b, cache, name, tokens, ss=None, rps=0, drop=None):
    """x2 wb^T + b (bf16): csrc/dense_gemm.hip with a plain epilogue (f32 bias b) where `tag` is routed to it (DENSE_HIP),
    else the BLAS library with the cache's compute-dtype bias.  ss / rps: the branch's stochastic-depth mask (dense_skip_scale),
    for the hand-written kernel only; drop: the probability it was drawn with (dense_cls_fold)."""
    if tag in DENSE_HIP:
        return ops.dense_gemm_nt(x2, wb, 0, bias=_f32(b), name=f"dense_nt_kernel<{name}>", tokens=tokens, sample_scale=ss,
                                 rows_per_sample=rps, fold_cls=ss is not None and dense_cls_fold(drop), drop=drop)
    return _linear_lib(x2, wb, None if b is None else cache.b)


def _gemm_dgrad(g2, wt, wb, shape, dtype, ss=None, rps=0, drop=None):
    """Input gradient g2 W as `shape` in `dtype`: csrc/dense_gemm.hip on the transposed copy wt where the cache made one (the
    input gradient is routed to it), else the BLAS library on wb.  ss / rps: the mask under which g2's rows of a dropped sample
    are exactly zero (dense_skip_scale), for the hand-written kernel only; drop: the probability it was drawn with."""
    gx = (ops.dense_gemm_nt(g2, wt, 0, name="dense_nt_kernel<dgrad>", tokens=_tok(shape), sample_scale=ss, rows_per_sample=rps,
                            fold_cls=ss is not None and dense_cls_fold(drop))
          if wt is not None else _mm_lib(g2, wb))
    return gx.view(shape).to(dtype)


def _resid_tail_fwd(ctx, x, tag, a2, wb, b, cache, tokens, g32, rs32, rps, nw, nb, neps, rows_to, stream, ds, drop=None):
    """out = x + rs * gamma * br with br = a2 wb^T + b, the GEMM `tag` (proj / fc2): the tail of both branches of a standard
    block.  neps is not None: the residual add and LayerNorm(out; nw, nb, neps) in bf16 as one row pass -> (out, yn).
    rows_to: x are compact rows of `stream`, the result goes back into it through the row map -> stream.
    ds: rs32 as the sample mask of the GEMM (dense_skip_scale): br meets rs = 0 in every row of a dropped sample.
    drop: the probability rs was drawn with, where the caller knows it (dense_cls_fold).
    Returns (the node's outputs, the tensors _resid_tail_bwd wants back from ctx.save_for_backward)."""
    ctx.rows_to, ctx.x_shape = rows_to, x.shape
    ctx.tail = (neps is not None, rps, b is not None, nw is not None, nb is not None)
    x2 = x.view(-1, wb.shape[0])
    if neps is None and rows_to is None and tag in DENSE_HIP and DENSE_RESID_FUSED:
        br, out = ops.dense_gemm_nt(a2, wb, 2, bias=_f32(b), gamma=g32, rs=rs32, rps=rps, x=x2, name="dense_nt_kernel<resid>")
        return out.view(x.shape), (br, g32, rs32)
    br = _gemm_fwd(tag, a2, wb, b, cache, tag, tokens, ds, rps, drop)
    if neps is not None:
        nw32, nb32 = _f32(nw), _f32(nb)
        out, yn, stats = ops.dense_resid_layernorm_fwd(x2, br, g32, rs32, rps, nw32, nb32, neps, torch.bfloat16,
                                                       skip_yb=ROW_INPLACE and ROW_SKIP_DROPPED)
        ctx.set_materialize_grads(False)
        yn = yn.view(x.shape)
        row_skip_attach(ctx, yn)
        return (out.view(x.shape), yn), (br, g32, rs32, out, stats, nw32)
    if rows_to is not None:
        ops.scale_residual_fwd_rows_(stream, rows_to.rowmap, x2, br, g32, rs32, rps)
        ctx.mark_dirty(stream)
        return stream, (br, g32, rs32, rows_to.rowmap)
    return ops.scale_residual_fwd(x2, br, g32, rs32, rps).view(x.shape), (br, g32, rs32)


def _resid_tail_bwd(ctx, tail, gout, gyn, want_norm):
    """Backward of _resid_tail_fwd.  tail: what it handed to save_for_backward; gyn: the cotangent of the next-norm output;
    want_norm: the norm's parameters want gradients.  Returns (stream cotangent - None under rows_to, where it travels
    through rows_to.link.g -, cotangent of br, d gamma, column sums of that cotangent = the bias gradient, d nw, d nb)."""
    norm, rps, has_b, has_nw, has_nb = ctx.tail
    br, g32, rs32, *rest = tail
    has_gamma = g32 is not None
    dnw = dnb = gbr = None
    if norm:
        out, stats, nw32 = rest
        if gyn is not None:      # LayerNorm backward with the residual cotangent added in the same pass
            want = has_nw and want_norm
            dres = None if gout is None else _c(gout.float()).view(out.shape)
            g2 = _c(gyn).view(out.shape)
            if LN_TAIL_FUSED and ops.dense_ln_bwd_tail_ok(g2, br, out.shape[-1]):
                ns, nrps = row_skip_get(ctx, g2.shape[0])
                mine = dres is not None and STREAM_GRADS.take(dres)    # (always asked: the entry is this node's to consume)
                gout, dnw, dnb, gbr, dgamma, colsum = ops.dense_layernorm_bwd_tail(
                    g2, out, nw32, stats, dres, br, g32, rs32, rps, want_param_grads=want, want_gamma=has_gamma,
                    want_colsum=has_b, sample_scale=ns, rows_per_sample=nrps, inplace=mine and ns is not None)
                STREAM_GRADS.offer(gout)                               # allocated there, or the owned buffer updated in place
            else:
                gout, dnw, dnb = ops.dense_layernorm_bwd(g2, out, nw32, stats, dres, want_param_grads=want)
            dnw, dnb = (dnw if has_nw else None), (dnb if has_nb else None)
    elif ctx.rows_to is not None:
        gout = _c(gout.float())
        ctx.rows_to.link.g = gout             # the LayerNorm of this branch edits it in place and hands it on
        gbr, dgamma, colsum = ops.scale_residual_bwd(gout, br, g32, rs32, rps, want_gamma=has_gamma, want_colsum=has_b,
                                                     rowmap=rest[0])
    if gbr is None:
        gout = _c(gout.float())
        gbr, dgamma, colsum = ops.scale_residual_bwd(gout.view(br.shape), br, g32, rs32, rps, want_gamma=has_gamma,
                                                     want_colsum=has_b)
    gx = None if ctx.rows_to is not None else gout.view(ctx.x_shape)
    return gx, gbr, dgamma, colsum, dnw, dnb


class DenseLinearNTFn(torch.autograd.Function):
    """nn.Linear (bf16 operands, f32 accumulate, f32 bias added before the one rounding to bf16): forward and input
    gradient on csrc/dense_gemm.hip.  deit/vit.py:33 (``self.qkv(x)``)."""

    @staticmethod
    def forward(ctx, x, w, b, cache, tag, pair=None, rs=None, rps=0, drop=None):
        """rs / rps: the stochastic-depth factor of the branch this projection opens and the rows per entry, where EVERYTHING
        computed from the output is multiplied by it (the qkv projection of vit.Attention.forward_fused) - the cotangent rows
        of a dropped sample are then zero and the weight gradient may skip them (wgrad_skip_scale).  drop: the probability rs
        was drawn with (dense_cls_fold)."""
        ctx.pair = pair
        ctx.drop = drop
        ctx.wparam = w
        xb = _c(x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16))
        wb, wt = cache.get_nt(w, b, ("d" + tag) in DENSE_HIP and ctx.needs_input_grad[0])
        x2 = xb.reshape(-1, wb.shape[1])
        mask = whole_sample_mask(rs, rps, x2.shape[0])
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        y = _gemm_fwd(tag, x2, wb, b, cache, "plain", _tok(x.shape), ds, rps, drop)
        ss = mask if WGRAD_SKIP_DROPPED else None
        # zero cotangent rows in (the attention backward of dO = 0), zero input-gradient rows out: the bias column sums and the
        # backward of the norm that produced x may skip them
        rk = mask if ROW_SKIP_DROPPED else None
        row_skip_fill(x, rk, rps, x2.shape[0])
        ctx.rps = rps
        ctx.save_for_backward(x2, wb, wt, ss, ds, rk)  # wt is None unless the input gradient is routed to the HIP kernel
        ctx.meta = (b is not None, x.dtype, x.shape, tag)
        return y.view(*x.shape[:-1], wb.shape[0])

    @staticmethod
    def backward(ctx, gy):
        x2, wb, wt, ss, ds, rk = ctx.saved_tensors
        has_b, x_dtype, x_shape, tag = ctx.meta
        g2 = _c(gy).reshape(-1, wb.shape[0])
        gx = _gemm_dgrad(g2, wt, wb, x_shape, x_dtype, ds, ctx.rps, ctx.drop) if ctx.needs_input_grad[0] else None
        gb = None
        if has_b:
            gb = (ops.dense_colsum(g2, rk, ctx.rps)
                  if g2.is_cuda and g2.dtype == torch.bfloat16 and g2.shape[1] % 8 == 0
                  else g2.sum(0, dtype=torch.float32))
        pair = ctx.pair
        if pair is not None and pair.pending is not None:
            pg, px = pair.pending[0], pair.pending[1]
            if (_pair_ready(pair, g2, x2) and pg.shape[0] == g2.shape[0] and px.shape[1] == x2.shape[1]
                    and ops.dense_wgrad_pair_ok(g2.shape[0], g2.shape[1], pg.shape[1], x2.shape[1])):
                pg, px, pdw, landed, pss, prps = pair.take()
                dest = ops.grad_dest(ctx.wparam, (g2.shape[1], x2.shape[1]))
                # one mask for both problems: only where both halves carry the same factors
                both = ss if (ss is not None and pss is not None and prps == ctx.rps and pss.data_ptr() == ss.data_ptr()
                              and pss.numel() == ss.numel()) else None
                dw, _ = ops.dense_wgrad_tn_pair(g2, x2, pg, px, dw1=pdw, dw0=dest, sample_scale=both, rows_per_sample=ctx.rps)
                ops.grad_written(landed, ctx.wparam if dest is not None else None)
                return gx, dw, gb, None, None, None, None, None, None
            pair.flush()
        return gx, _wgrad_lib(g2, x2, ctx.wparam, ss, ctx.rps), gb, None, None, None, None, None, None


class DenseProjResidFn(torch.autograd.Function):
    """out = x + rs * gamma * (a W^T + b): the tail of a standard-block branch (deit/vit.py:131-134) as ONE GEMM with a
    fused epilogue; backward = one HIP row pass (gy, d gamma, bias gradient) + the input-gradient GEMM."""

    @staticmethod
    def forward(ctx, x, a, w, b, gamma, rs, rps, cache, nw=None, nb=None, neps=None, pair=None, rows_to=None, stream=None,
                drop=None):
        """neps is not None: also return LayerNorm(out; nw, nb, neps) in bf16 - the norm that opens the next branch - from
        the same row pass that adds the residual (NEXT_NORM_FUSED).  rows_to (RowsTo; stream = rows_to.stream, passed as a
        tensor so that autograd sees the in-place edit): x are compact rows of the stream, the result goes back into it.
        drop: the probability rs was drawn with (dense_cls_fold)."""
        ctx.pair = pair
        ctx.drop = drop
        ctx.wparam = w
        x = _c(x)
        ab = _c(a if a.dtype == torch.bfloat16 else a.to(torch.bfloat16))
        wb, wt = cache.get_nt(w, b, "dproj" in DENSE_HIP and ctx.needs_input_grad[1])
        a2 = ab.reshape(-1, wb.shape[1])
        rs32 = _f32(rs)
        outs, tail = _resid_tail_fwd(ctx, x, "proj", a2, wb, b, cache, _tok(a.shape), _f32(gamma), rs32, rps,
                                     nw, nb, neps, rows_to, stream, dense_skip_scale(rs32, rps, a2.shape[0], rows_to), drop)
        ctx.save_for_backward(a2, wb, wt, *tail)
        ctx.meta = (a.dtype, a.shape)
        return outs

    @staticmethod
    def backward(ctx, gout, gyn=None):
        a2, wb, wt, *tail = ctx.saved_tensors
        a_dtype, a_shape = ctx.meta
        gx, gy, dgamma, colsum, dnw, dnb = _resid_tail_bwd(ctx, tail, gout, gyn,
                                                           ctx.needs_input_grad[8] or ctx.needs_input_grad[9])
        rps = ctx.tail[1]
        mask = whole_sample_mask(tail[2], rps, gy.shape[0], ctx.rows_to)  # gy = rs * gamma * gout: zero rows where rs is 0
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        ga = _gemm_dgrad(gy, wt, wb, a_shape, a_dtype, ds, rps, ctx.drop) if ctx.needs_input_grad[1] else None
        ss = mask if WGRAD_SKIP_DROPPED else None
        if _pair_ready(ctx.pair, gy, a2) and ops.dense_wgrad_ok(gy.shape[0], gy.shape[1], a2.shape[1]):
            dw = ctx.pair.park(gy, a2, ctx.wparam, ss, rps)   # written by the qkv weight gradient's launch (or at the end of the pass)
        else:
            dw = _wgrad_lib(gy, a2, ctx.wparam, ss, rps)
        return gx, ga, dw, colsum, dgamma, None, None, None, dnw, dnb, None, None, None, None, None


class DenseMlpFn(torch.autograd.Function):
    """x + rs * gamma * fc2(gelu(fc1(y))) of a standard block (timm Mlp inside deit/vit.py:131-134).  Per GEMM, routed by
    DENSE_HIP: fc1 with bias + exact-erf GELU in the epilogue (pre-activation kept for the backward), fc2 with bias, layer
    scale, stochastic depth and the f32 residual in the epilogue, fc2's input gradient with GELU' in its epilogue, fc1's
    input gradient; otherwise the BLAS library with the row kernels of csrc/dense.hip around it.  Weight gradients:
    csrc/dense_wgrad.hip (WGRAD_HIP)."""

    @staticmethod
    def forward(ctx, y, x, w1, b1, w2, b2, gamma, rs, rps, c1, c2, nw=None, nb=None, neps=None, rows_to=None, stream=None,
                drop=None):
        """neps is not None: also return LayerNorm(out; nw, nb, neps) in bf16 (the NEXT block's norm1) from the row pass
        that adds the residual.  rows_to / stream / drop: as in DenseProjResidFn."""
        ctx.wparams = (w1, w2)
        ctx.drop = drop
        x = _c(x)
        yb = _c(y if y.dtype == torch.bfloat16 else y.to(torch.bfloat16))
        need_t = any(ctx.needs_input_grad[:2])            # (an inference pass - the DINOv2 teacher - never transposes)
        w1b, w1t = c1.get_nt(w1, b1, "dfc1" in DENSE_HIP and need_t)
        w2b, w2t = c2.get_nt(w2, b2, "dfc2" in DENSE_HIP and need_t)
        y2 = yb.reshape(-1, w1b.shape[1])
        g32, rs32 = _f32(gamma), _f32(rs)
        # GELU_FACTOR: fc1's epilogue leaves gelu'(h) (bf16) instead of h; fc2's input gradient multiplies by it (modes 4 / 5 of
        # octic_dense_gemm_nt) - the erf of the backward epilogue is computed once, in the forward, beside gelu's
        factor = GELU_FACTOR and "fc1" in DENSE_HIP and w2t is not None
        ctx.factor = factor
        # fc1's outputs of a dropped sample are read by fc2 (whose output meets rs = 0) and by gradients whose dY rows are zero
        mask = whole_sample_mask(rs32, rps, y2.shape[0], rows_to)
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        # fc1's input gradient is dh W1 with dh = gelu' * (gbr W2) and gbr = rs * gamma * gout: zero rows where rs is 0, so
        # the backward of the norm that produced y may skip them
        row_skip_fill(y, mask if ROW_SKIP_DROPPED else None, rps, y2.shape[0])
        if "fc1" in DENSE_HIP and not any(ctx.needs_input_grad):
            # no backward will come (inference, the DINOv2 teacher): gelu(h) only, nothing kept (mode 6)
            a = ops.dense_gemm_nt(y2, w1b, 6, bias=_f32(b1), name="dense_nt_kernel<gelu-only>", tokens=_tok(y.shape),
                                  sample_scale=ds, rows_per_sample=rps)
            h = a
        elif "fc1" in DENSE_HIP:
            h, a = ops.dense_gemm_nt(y2, w1b, 4 if factor else 1, bias=_f32(b1), name="dense_nt_kernel<gelu>",
                                     tokens=_tok(y.shape), sample_scale=ds, rows_per_sample=rps, drop=drop)
        else:
            h = _linear_lib(y2, w1b, None if b1 is None else c1.b)
            a = torch.nn.functional.gelu(h)
        outs, tail = _resid_tail_fwd(ctx, x, "fc2", a, w2b, b2, c2, _tok(y.shape), g32, rs32, rps,
                                     nw, nb, neps, rows_to, stream, ds, drop)
        ctx.save_for_backward(y2, h, a, w1b, w1t, w2b, w2t, *tail)
        ctx.meta = (b1 is not None, y.dtype, y.shape)
        return outs

    @staticmethod
    def backward(ctx, gout, gyn=None):
        y2, h, a, w1b, w1t, w2b, w2t, *tail = ctx.saved_tensors
        has_b1, y_dtype, y_shape = ctx.meta
        gx, gbr, dgamma, db2, dnw, dnb = _resid_tail_bwd(ctx, tail, gout, gyn,
                                                         ctx.needs_input_grad[11] or ctx.needs_input_grad[12])
        rps = ctx.tail[1]
        mask = whole_sample_mask(tail[2], rps, gbr.shape[0], ctx.rows_to)  # gbr = rs * gamma * gout: zero rows where rs is 0
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        if w2t is not None:
            md = 5 if ctx.factor else 3
            if has_b1:                                                                  # gelu'(h) * (gbr W2), + db1
                dh, db1 = ops.dense_gemm_nt(gbr, w2t, md, h=h, name="dense_nt_kernel<dgelu>", want_colsum=True,
                                            tokens=_tok(y_shape), sample_scale=ds, rows_per_sample=rps, drop=ctx.drop)
            else:
                dh, db1 = ops.dense_gemm_nt(gbr, w2t, md, h=h, name="dense_nt_kernel<dgelu>", tokens=_tok(y_shape),
                                            sample_scale=ds, rows_per_sample=rps, drop=ctx.drop), None
        else:
            dh, db1 = ops.dense_gelu_bwd(h, _mm_lib(gbr, w2b), want_colsum=has_b1)
        ss = mask if WGRAD_SKIP_DROPPED else None                         # gbr = rs * gamma * gout, dh = gelu' * (gbr W2)
        gw2 = _wgrad_lib(gbr, a, ctx.wparams[1], ss, rps)
        gw1 = _wgrad_lib(dh, y2, ctx.wparams[0], ss, rps)
        gy = _gemm_dgrad(dh, w1t, w1b, y_shape, y_dtype, ds, rps, ctx.drop) if ctx.needs_input_grad[0] else None   # dh = gelu' * 0
        return gy, gx, gw1, db1, gw2, db2, dgamma, None, None, None, None, dnw, dnb, None, None, None, None


class DenseSwigluFn(torch.autograd.Function):
    """x + rs * gamma * w3(silu(x1) * x2) with (x1, x2) = w12(y).chunk(2, -1): DINOv2's SwiGLU FFN inside a standard block
    (dinov2/layers/swiglu_ffn.py:30-34, block.py:94), the counterpart of DenseMlpFn.  w12 is a plain-epilogue GEMM on
    csrc/dense_gemm.hip where "fc1" is routed (DENSE_HIP) and the kernel takes the shape, else the BLAS library; the gate and
    its backward (with w12's bias gradient on the side) are the row kernels of csrc/swiglu.hip either way; w3 runs through the
    shared residual tail as "fc2".  Weight gradients: csrc/dense_wgrad.hip (WGRAD_HIP)."""

    @staticmethod
    def forward(ctx, y, x, w12, b12, w3, b3, gamma, rs, rps, c1, c2, nw=None, nb=None, neps=None, rows_to=None, stream=None):
        """The trailing arguments are DenseMlpFn's."""
        ctx.wparams = (w12, w3)
        x = _c(x)
        yb = _c(y if y.dtype == torch.bfloat16 else y.to(torch.bfloat16))
        H, D = w3.shape[1], w12.shape[1]
        y2 = yb.reshape(-1, D)
        M = y2.shape[0]
        need_t = any(ctx.needs_input_grad[:2])            # (an inference pass - the DINOv2 teacher - never transposes)
        # per GEMM: routed and a shape the hand-written kernel takes (others: the library, as vit.Mlp falls back)
        hip12 = "fc1" in DENSE_HIP and ops.dense_gemm_ok(M, 2 * H, D)
        hip3 = "fc2" in DENSE_HIP and ops.dense_gemm_ok(M, w3.shape[0], H)
        w12b, w12t = c1.get_nt(w12, b12, need_t and "dfc1" in DENSE_HIP and ops.dense_gemm_ok(M, D, 2 * H))
        w3b, w3t = c2.get_nt(w3, b3, need_t and "dfc2" in DENSE_HIP and ops.dense_gemm_ok(M, H, w3.shape[0]))
        g32, rs32 = _f32(gamma), _f32(rs)
        # x12 of a dropped sample is read by the gate alone, whose output meets rs = 0 behind w3 and zero dY rows in the gradients
        mask = whole_sample_mask(rs32, rps, M, rows_to)
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        # w12's input gradient is dx12 W12 with dx12 = gate'(x12) * (gbr W3) and gbr = rs * gamma * gout: zero rows where rs is 0
        row_skip_fill(y, mask if ROW_SKIP_DROPPED else None, rps, M)
        x12 = _gemm_fwd("fc1" if hip12 else "fc1-library", y2, w12b, b12, c1, "plain", _tok(y.shape), ds, rps)
        a = ops.swiglu_fwd(x12, H)
        outs, tail = _resid_tail_fwd(ctx, x, "fc2" if hip3 else "fc2-library", a, w3b, b3, c2, _tok(y.shape), g32, rs32, rps,
                                     nw, nb, neps, rows_to, stream, ds)
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(y2, x12, a, w12b, w12t, w3b, w3t, *tail)
        ctx.meta = (b12 is not None, y.dtype, y.shape)
        return outs

    @staticmethod
    def backward(ctx, gout, gyn=None):
        y2, x12, a, w12b, w12t, w3b, w3t, *tail = ctx.saved_tensors
        has_b12, y_dtype, y_shape = ctx.meta
        gx, gbr, dgamma, db3, dnw, dnb = _resid_tail_bwd(ctx, tail, gout, gyn,
                                                         ctx.needs_input_grad[11] or ctx.needs_input_grad[12])
        rps = ctx.tail[1]
        mask = whole_sample_mask(tail[2], rps, gbr.shape[0], ctx.rows_to)  # gbr = rs * gamma * gout: zero rows where rs is 0
        ds = mask if DENSE_NT_SKIP_DROPPED else None
        ga = _gemm_dgrad(gbr, w3t, w3b, (*y_shape[:-1], a.shape[1]), a.dtype, ds, rps)
        dx12, db12 = ops.swiglu_bwd(x12, ga, want_colsum=has_b12)
        ss = mask if WGRAD_SKIP_DROPPED else None                         # dx12 = gate' * (gbr W3): zero rows with gbr's
        gw3 = _wgrad_lib(gbr, a, ctx.wparams[1], ss, rps)
        gw12 = _wgrad_lib(dx12, y2, ctx.wparams[0], ss, rps)
        gy = _gemm_dgrad(dx12, w12t, w12b, y_shape, y_dtype, ds, rps) if ctx.needs_input_grad[0] else None
        return gy, gx, gw12, db12, gw3, db3, dgamma, None, None, None, None, dnw, dnb, None, None, None


# -------------------------------------------------------------------------------------- hand-off
# ------------------------------------------------------------------ input rows of the DINO / iBOT heads (ssl.HEAD_HIP)
class HeadRowsFn(torch.autograd.Function):
    """The input rows of a DINO / iBOT head call (dinov2/train/ssl_meta_arch.py:226-267: new_zeros + index_select + copy_ + cat)
    as ONE gather launch: out [rows_out, D] in the sources' dtype, source s - [n, D], or [B, P, D] read as its B * P rows - taken
    through specs[s] = (idx or None, out_row0) into out[out_row0 : out_row0 + n], every other row +0.  Backward: one scatter
    launch of the cotangent rows into the sources' gradients (plain stores: the indices are distinct, as mask_indices_list is),
    an indexed source's gradient zero-filled once."""

    @staticmethod
    def forward(ctx, rows_out, specs, *sources):
        out = torch.empty((rows_out, sources[0].shape[-1]), dtype=sources[0].dtype, device=sources[0].device)
        ops.head_rows([(s.detach(), idx, r0) for s, (idx, r0) in zip(sources, specs)], out)
        ctx.specs = specs
        ctx.shapes = [s.shape for s in sources]
        return out

    @staticmethod
    def backward(ctx, g):
        g2 = ops._aligned_rows2d(g, "head_rows")
        grads, segs = [], []
        for need, shape, (idx, r0) in zip(ctx.needs_input_grad[2:], ctx.shapes, ctx.specs):
            if not need:
                grads.append(None)
                continue
            gs = (torch.empty if idx is None else torch.zeros)(shape, dtype=g2.dtype, device=g2.device)
            grads.append(gs)
            segs.append((gs, idx, r0))
        if segs:
            ops.head_rows(segs, g2, scatter=True)
        return (None, None, *grads)


def head_rows_ok(rows_out, specs, sources):
    """HeadRowsFn takes these sources: GPU tensors of one f32 / bf16 dtype and width, [n, D] or [B, P, D] with unit column stride
    and 16-byte aligned rows, at least one row each, int64 indices on the device, at most four of them, not under torch.compile
    tracing."""
    if torch.compiler.is_compiling() or not 1 <= len(sources) <= ops.HEAD_ROWS_MAX_SEGMENTS or rows_out < 1:
        return False
    s0 = sources[0]
    D, es = s0.shape[-1], s0.element_size()
    if not s0.is_cuda or s0.dtype not in (torch.float32, torch.bfloat16) or D < 8 or D % 8:
        return False
    for s, (idx, _) in zip(sources, specs):
        if (s.device != s0.device or s.dtype != s0.dtype or s.dim() not in (2, 3) or s.shape[-1] != D or s.numel() == 0
                or s.stride(-1) != 1 or s.data_ptr() % 16 or any((ld * es) % 16 for ld in s.stride()[:-1])):
            return False
        if idx is not None and not (idx.is_cuda and idx.dtype == torch.int64 and idx.dim() == 1 and idx.is_contiguous()):
            return False
    return True


# ------------------------------------------------------------------ the DINO / iBOT head itself (ssl.DINO_HEAD_HIP)
# dinov2/layers/dino_head.py:36-41 under bf16 autocast: the MLP on csrc/dense_gemm.hip (bias / GELU epilogues, GELU' and the bias
# column sums in the input-gradient GEMMs), F.normalize as one row kernel each way and the weight-normed prototype layer straight
# from weight_g / weight_v (csrc/dino_norm.hip).  The bf16 operands are made per call - in a training step every head runs once
# per parameter version, so a cache could not hit - and nothing here keeps state between calls: a raw-pointer write of the fused
# optimizer or of update_teacher is seen by the next call.  Gradients leave as ordinary autograd outputs (f32, the parameters'
# shapes).  NEVER capture a backward pass through a DINOHead in a hipGraph or run it on a side stream: the stock module's
# last_layer.weight keeps the AccumulateGrad nodes of weight_g / weight_v alive from its constructor on (NOTES 'DINO head').
class L2NormRowsFn(torch.autograd.Function):
    """F.normalize(x, dim=-1, p=2, eps) of x [rows, D] (f32 / bf16) in x's dtype: one row kernel each way (ops.l2norm_rows)."""

    @staticmethod
    def forward(ctx, x, eps=1e-12):
        x2 = ops._aligned_rows2d(x.detach(), "L2NormRowsFn")
        y, inv = ops.l2norm_rows(x2, eps)
        ctx.save_for_backward(x2, inv)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        x2, inv = ctx.saved_tensors
        return ops.l2norm_rows_bwd(ops._aligned_rows2d(g, "L2NormRowsFn"), x2, inv, ctx.eps), None


def _bf16_rows(t):
    return _c(t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16))


class WeightNormLinearFn(torch.autograd.Function):
    """x [rows, K] @ (weight_g weight_v / ||weight_v||_row)^T of nn.utils.weight_norm(nn.Linear(K, N, bias=False)) in bf16: one
    ops.weight_norm_prep launch makes both GEMM operands from the f32 parameters (the transposed one only where x wants a
    gradient), the NT GEMM of csrc/dense_gemm.hip; backward: the input-gradient GEMM on the transposed operand, the TN weight
    gradient in f32 (_wgrad_lib), then ops.weight_norm_bwd -> (dv, dg)."""

    @staticmethod
    def forward(ctx, x, weight_g, weight_v):
        xb = _bf16_rows(x.detach())
        g32, v32 = _c(weight_g.detach()), _c(weight_v.detach())
        w, wt, norms = ops.weight_norm_prep(v32, g32, want_wt=ctx.needs_input_grad[0])
        y = ops.dense_gemm_nt(xb, w, 0, name="dense_nt_kernel<prototypes>")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(xb, wt, norms, g32, v32)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, gy):
        xb, wt, norms, g32, v32 = ctx.saved_tensors
        g2 = _bf16_rows(gy)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.dense_gemm_nt(g2, wt, 0, name="dense_nt_kernel<dprototypes>").to(ctx.x_dtype)
        dg = dv = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dv, dg = ops.weight_norm_bwd(_c(_wgrad_lib(g2, xb)), v32, g32, norms)
        return dx, dg, dv


class DinoMlpFn(torch.autograd.Function):
    """The head's MLP - nl Linear layers with exact GELU between them - on x [rows, K0] in bf16: params = (w0, b0, w1, b1, ...),
    a missing bias None.  Forward: bias + GELU in the GEMM epilogue with the pre-activation kept (mode 1; mode 6 where no backward
    will come: the teacher), the last layer plain.  Backward, last layer first: the bias gradient of the last layer as a column
    sum, every other one out of the GELU' epilogue of the input-gradient GEMM behind it (mode 3), weight gradients in f32
    (_wgrad_lib)."""

    @staticmethod
    def forward(ctx, x, nl, *params):
        a = _bf16_rows(x.detach())
        need = any(ctx.needs_input_grad)
        acts, pre, wbs = [], [], []
        for i in range(nl):
            w, b = params[2 * i], params[2 * i + 1]
            wb = _c(w.detach().to(torch.bfloat16))                 # one cast per weight and call
            acts.append(a)
            wbs.append(wb)
            if i == nl - 1:
                a = ops.dense_gemm_nt(a, wb, 0, bias=_f32(b), name="dense_nt_kernel<head-plain>")
            elif need:
                h, a = ops.dense_gemm_nt(a, wb, 1, bias=_f32(b), name="dense_nt_kernel<head-gelu>")
                pre.append(h)
            else:
                a = ops.dense_gemm_nt(a, wb, 6, bias=_f32(b), name="dense_nt_kernel<head-gelu-only>")
        if need:
            ctx.save_for_backward(*acts, *pre, *wbs)
        ctx.nl, ctx.x_dtype = nl, x.dtype
        ctx.has_b = [params[2 * i + 1] is not None for i in range(nl)]
        return a

    @staticmethod
    def backward(ctx, gy):
        nl = ctx.nl
        saved = ctx.saved_tensors
        acts, pre, wbs = saved[:nl], saved[nl:2 * nl - 1], saved[2 * nl - 1:]
        g = _bf16_rows(gy)
        grads = [None] * (2 * nl)
        db = ops.dense_colsum(g) if ctx.has_b[nl - 1] else None
        dx = None
        for i in reversed(range(nl)):
            grads[2 * i] = _wgrad_lib(g, acts[i])
            grads[2 * i + 1] = db
            if i > 0:
                wt = wbs[i].t().contiguous()
                if ctx.has_b[i - 1]:
                    g, db = ops.dense_gemm_nt(g, wt, 3, h=pre[i - 1], name="dense_nt_kernel<head-dgelu>", want_colsum=True)
                else:
                    g, db = ops.dense_gemm_nt(g, wt, 3, h=pre[i - 1], name="dense_nt_kernel<head-dgelu>"), None
            elif ctx.needs_input_grad[0]:
                dx = ops.dense_gemm_nt(g, wbs[0].t().contiguous(), 0, name="dense_nt_kernel<head-dgrad>").to(ctx.x_dtype)
        return (dx, None, *grads)


def _dino_head_linears(head):
    """The nn.Linear layers of head.mlp where it is Linear (GELU Linear)* with exact GELUs, else None."""
    mlp = head.mlp
    mods = [mlp] if isinstance(mlp, torch.nn.Linear) else list(mlp) if isinstance(mlp, torch.nn.Sequential) else None
    if not mods or len(mods) % 2 == 0:
        return None
    for i, m in enumerate(mods):
        if i % 2 == 0 and type(m) is not torch.nn.Linear:
            return None
        if i % 2 == 1 and not (type(m) is torch.nn.GELU and m.approximate == "none"):
            return None
    return mods[0::2]


def dino_head_ok(head, x):
    """The one routing predicate of the head's engine path (dino_head_forward): x [rows >= 1, in_dim] f32 / bf16 on the GPU under
    bf16 autocast, not under torch.compile tracing; a head without BatchNorm whose parameters are f32 on x's device; and EVERY
    GEMM of the head - MLP layers and prototypes, forward (K = in_features) and input gradient (K = out_features) - a shape
    ops.dense_gemm_ok takes, the bottleneck a width the row kernels take.  One refusal and the whole head keeps the stock path."""
    if torch.compiler.is_compiling() or not isinstance(x, torch.Tensor) or not x.is_cuda or x.dim() != 2 or x.shape[0] < 1:
        return False
    if x.dtype not in (torch.float32, torch.bfloat16):
        return False
    if not torch.is_autocast_enabled() or torch.get_autocast_gpu_dtype() != torch.bfloat16:
        return False
    lins = _dino_head_linears(head)
    last = getattr(head, "last_layer", None)
    wg, wv = getattr(last, "weight_g", None), getattr(last, "weight_v", None)
    if lins is None or wg is None or wv is None or getattr(last, "bias", None) is not None:
        return False
    rows = x.shape[0]
    tensors = [t for m in lins for t in (m.weight, m.bias) if t is not None] + [wg, wv]
    if any(t.device != x.device or t.dtype != torch.float32 for t in tensors):
        return False
    if lins[0].in_features != x.shape[1] or wv.dim() != 2 or tuple(wg.shape) != (wv.shape[0], 1):
        return False
    shapes = [(m.out_features, m.in_features) for m in lins] + [tuple(wv.shape)]
    if any(a[0] != b[1] for a, b in zip(shapes, shapes[1:])):
        return False
    if not all(ops.dense_gemm_ok(rows, N, K) and ops.dense_gemm_ok(rows, K, N) for N, K in shapes):
        return False
    P, D = shapes[-1]
    return bool(ops.l2norm_ok(rows, D) and ops.weight_norm_ok(P, D))


def dino_head_forward(head, x):
    """ssl.DINOHead.forward on the engine (check dino_head_ok first): reads last_layer.weight_g / weight_v directly and never
    touches last_layer.weight."""
    lins = _dino_head_linears(head)
    y = DinoMlpFn.apply(x, len(lins), *[t for m in lins for t in (m.weight, m.bias)])
    y = L2NormRowsFn.apply(y, 1e-12)
    return WeightNormLinearFn.apply(y, head.last_layer.weight_g, head.last_layer.weight_v)


class HandoffCatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c, out_dtype):
        ctx.c, ctx.in_dtype = c, x.dtype
        return ops.handoff_cat_fwd(_c(x.float()), c, out_dtype)

    @staticmethod
    def backward(ctx, g):
        return ops.handoff_cat_bwd(g, ctx.c).to(ctx.in_dtype), None, None


class PowerSpectrumFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, c, out_dtype):
        x = _c(x.float())
        ctx.save_for_backward(x)
        ctx.c = c
        return ops.power_spectrum_fwd(x, c, out_dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return ops.power_spectrum_bwd(g, x, ctx.c), None, None


# ------------------------------------------------------------------------------------------ lift
class LiftFn(torch.autograd.Function):
    """tokens[b, tok0+n, :] = patches(img)[b,n,:] @ Wfull^T + bias_full + pos[n,:] ; tokens[b, :tok0] = cls."""

    @staticmethod
    def forward(ctx, img, wfull, bias_full, pos, cls_row, p, dtype):
        B, Cin, Hh, Ww = img.shape
        D, K = wfull.shape
        Kpad = (K + 7) // 8 * 8
        n_p = (Hh // p) * (Ww // p)
        tok0 = 0 if cls_row is None else 1
        patches = ops.im2col(img, p, Kpad, dtype)
        wpad = torch.zeros((D, Kpad), dtype=dtype, device=img.device)
        wpad[:, :K] = wfull.detach()
        out = torch.empty((B, tok0 + n_p, D), dtype=torch.float32, device=img.device)
        ops.lift_gemm(patches, wpad, None if bias_full is None else _c(bias_full.detach().float()),
                      None if pos is None else _c(pos.detach().float()), out, B, n_p, tok0, Kpad, D)
        if tok0:
            out[:, 0] = cls_row.detach().float()
        ctx.save_for_backward(patches)
        ctx.meta = (B, n_p, tok0, K, Kpad, D, dtype, bias_full is not None, pos is not None)
        return out

    @staticmethod
    def backward(ctx, dout):
        (patches,) = ctx.saved_tensors
        B, n_p, tok0, K, Kpad, D, dtype, has_bias, has_pos = ctx.meta
        dtok = dout[:, tok0:]
        dcompact = _c(dtok.to(dtype)).reshape(B * n_p, D)
        dw = ops.lift_wgrad(patches, dcompact, Kpad, D)[:, :K]
        dpos = dtok.sum(0) if (has_pos or has_bias) else None
        dbias = dpos.sum(0) if has_bias else None
        dcls = dout[:, 0].sum(0) if tok0 else None
        return None, dw, dbias, dpos if has_pos else None, dcls, None, None


# ------------------------------------------------------------------------------------------ orbit invariants
class MaxFilterFn(torch.autograd.Function):
    """MaxFilteringInvariant on packed rows: out[t, d] = max_g x[t] . (A_g references[d]).  Saves x in the compute dtype, the
    winners (uint8) and the component planes of this call (R c 8 elements of the compute dtype)."""

    @staticmethod
    def forward(ctx, x, references, c, out_dtype):
        dt = compute_dtype(x)
        lead = x.shape[:-1]
        xc = _c(x.detach().reshape(-1, 8 * c).to(dt))
        refs = _c(references.detach().float())
        planes = ops.max_filter_prep(refs, dt)
        out, idx = ops.max_filter_fwd(xc, planes, c, out_dtype)
        ctx.save_for_backward(xc, idx, planes)
        ctx.meta = (c, x.dtype, references.dtype, lead)
        return out.view(*lead, refs.shape[0])

    @staticmethod
    def backward(ctx, g):
        xc, idx, planes = ctx.saved_tensors
        c, x_dtype, ref_dtype, lead = ctx.meta
        g = _c(g.reshape(idx.shape).to(xc.dtype))
        dx = dref = None
        if ctx.needs_input_grad[0]:
            dx = ops.max_filter_bwd_x(g, idx, planes, c).view(*lead, 8 * c).to(x_dtype)
        if ctx.needs_input_grad[1]:
            dref = ops.max_filter_bwd_ref(g, idx, xc, c).to(ref_dtype)
        return dx, dref, None, None


class CanonizeFn(torch.autograd.Function):
    """CanonizationInvariant on packed rows: out[t] = A_g x[t] for the g that maximises reference . (A_g x[t]), as the dense
    i-major row.  The reference only feeds the argmax: it gets no gradient.  Saves the winners alone."""

    @staticmethod
    def forward(ctx, x, reference, c, out_dtype):
        dt = compute_dtype(x)
        lead = x.shape[:-1]
        xc = _c(x.detach().reshape(-1, 8 * c).to(dt))
        out, idx = ops.canonize_fwd(xc, _c(reference.detach().float()), c, out_dtype)
        ctx.save_for_backward(idx)
        ctx.meta = (c, x.dtype, dt, lead)
        return out.view(*lead, 8 * c)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        c, x_dtype, dt, lead = ctx.meta
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        dx = ops.canonize_bwd(_c(g.reshape(-1, 8 * c)), idx, c, dt)
        return dx.view(*lead, 8 * c).to(x_dtype), None, None, None


# ------------------------------------------------------------------------------------------ polynomial invariants
class PolyInvariantFn(torch.autograd.Function):
    """PolynomialInvariant / ThirdOrderInvariant on packed float32 rows (map: "polynomial" | "third_order").  Saves x alone -
    for a contiguous float32 input that is the input itself, not a copy - and takes the cotangent in the dtype it arrives in
    (float32 or bfloat16)."""

    @staticmethod
    def forward(ctx, x, c, map, out_dtype):
        x = _c(x.float())
        ctx.save_for_backward(x)
        ctx.meta = (c, map)
        return ops.poly_invariant_fwd(x, c, map, out_dtype)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        c, map = ctx.meta
        if g.dtype not in (torch.float32, torch.bfloat16):
            g = g.float()
        return ops.poly_invariant_bwd(_c(g), x, c, map), None, None, None
