"""Raw (non-autograd) launches of the HIP engine on torch tensors.

torch is plumbing here: it owns device memory and the current HIP stream; every call goes straight
through the C ABI (include/octic_hip.h) via ctypes.  Tensors are described to the ABI as
``octic_view`` (5 base pointers + row strides), so both the reference's 5-tuple of separate tensors
and the engine's packed ``[B, T, 8c]`` rows are handled by the same kernels without a copy.
"""
import ctypes
import operator

import torch

from . import _lib
from ._lib import BF16, F32, OcticView, PtrArray5, check, lib

_DT = {torch.float32: F32, torch.bfloat16: BF16}
_DTN = {torch.float32: "f32", torch.bfloat16: "bf16"}


class KernelTimer:
    """Optional per-launch timing with HIP events on the stream the kernels are launched on (torch's current
    stream).  Disabled by default: zero overhead.  bench.py enables it over the timed steps to report the
    dominant kernel's achieved bytes/s against the HBM roofline."""

    def __init__(self):
        self.on = False
        self.records = []
        self.overhead_us = 0.0

    def enable(self):
        self.on, self.records = True, []
        # What an event pair reads with NOTHING between its two records (the second marker's own cost on the queue, ~1 us on
        # MI355X): subtracted from every bracket, so that ~1800 brackets per step do not add up to a millisecond of phantom
        # kernel time.  Median of 64 empty pairs on the current stream.
        pairs = []
        for _ in range(64):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        self.overhead_us = sorted(a.elapsed_time(b) * 1e3 for a, b in pairs)[len(pairs) // 2]

    def disable(self):
        self.on = False

    def start(self):
        if not self.on:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def stop(self, e0, name, alg_bytes, flops=0):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.records.append((name, e0, e1, alg_bytes, flops))

    def _agg(self):
        torch.cuda.synchronize()
        agg = {}
        for name, e0, e1, b, f in self.records:
            a = agg.setdefault(name, {"name": name, "launches": 0, "total_us": 0.0, "bytes": 0.0, "flops": 0.0})
            a["launches"] += 1
            a["total_us"] += max(0.0, e0.elapsed_time(e1) * 1e3 - self.overhead_us)
            a["bytes"] += b
            a["flops"] += f
        for a in agg.values():
            a["avg_us"] = a["total_us"] / a["launches"]
            a["alg_bytes_per_launch"] = a["bytes"] / a["launches"]
            a["flops_per_launch"] = a["flops"] / a["launches"]
        return agg

    @staticmethod
    def bound_of(name):
        """Roofline that bounds a kernel family: the attention kernels are MFMA/VALU-bound (q,k,v,o are read once,
        14 T^2 hd flops per head), every other kernel of the engine moves more bytes than it can compute on."""
        return "mfma" if name.startswith(("attn_", "dense_nt_kernel", "dense_tn_kernel", "dense_f32_n", "dense_f32_tn",
                                          "library_gemm")) else "hbm"

    def dominant(self, bound=None):
        agg = [a for a in self._agg().values() if bound is None or self.bound_of(a["name"]) == bound]
        return max(agg, key=lambda a: a["total_us"]) if agg else None

    def summary(self):
        out = {}
        for k, a in sorted(self._agg().items(), key=lambda kv: -kv[1]["total_us"]):
            us = a["avg_us"] or float("inf")      # (every launch at or below the event pair's own overhead: no rate to report)
            out[k] = {"launches": a["launches"], "total_us": round(a["total_us"], 1), "avg_us": round(a["avg_us"], 2),
                      "GBps": round(a["alg_bytes_per_launch"] / us / 1e3, 1)}
            if a["flops_per_launch"]:
                out[k]["TFLOPs"] = round(a["flops_per_launch"] / us / 1e6, 1)
        return out


KERNEL_TIMER = KernelTimer()


def dt_code(dtype):
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"octic engine supports float32 and bfloat16, got {dtype}") from None


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _require_cuda(t):
    if not t.is_cuda:
        raise RuntimeError("octic_vits_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")


def pview(t: torch.Tensor, c: int) -> OcticView:
    """View of a packed tensor [..., 8c] = [A1|A2|B1|B2|E_row0|E_row1]."""
    _require_cuda(t)
    if t.shape[-1] != 8 * c or not t.is_contiguous():
        raise ValueError(f"expected a contiguous packed tensor with last dim {8 * c}, got {tuple(t.shape)}")
    es, base, D = t.element_size(), t.data_ptr(), 8 * c
    v = OcticView()
    for i in range(4):
        v.ptr[i] = base + i * c * es
        v.ld[i] = D
    v.ptr[4] = base + 4 * c * es
    v.ld[4] = D
    return v


def _rows_ok(t, inner):
    """t viewed as rows of `inner` contiguous elements with one uniform row stride?"""
    lead = t.shape[:-len(inner)]
    st = t.stride()
    exp = 1
    for k in range(1, len(inner) + 1):
        if t.shape[-k] != inner[-k] or (st[-k] != exp and t.shape[-k] != 1):
            return False
        exp *= inner[-k]
    # leading dims must collapse onto a single stride
    ld = st[len(lead) - 1] if lead else exp
    acc = ld
    for k in range(len(lead) - 1, -1, -1):
        if t.shape[k] != 1 and st[k] != acc:
            return False
        acc *= t.shape[k]
    return True


def tview(xs, c: int):
    """View of a reference-style 5-tuple (A1..B2: [..., c]; E: [..., 2, 2c]).  Returns (view, keepalive)."""
    keep = []
    v = OcticView()
    for i in range(5):
        t = xs[i]
        _require_cuda(t)
        inner = (c,) if i < 4 else (2, 2 * c)
        if tuple(t.shape[-len(inner):]) != inner:
            raise ValueError(f"irrep {i}: expected trailing shape {inner}, got {tuple(t.shape)}")
        if not _rows_ok(t, inner):
            t = t.contiguous()
        keep.append(t)
        nlead = t.dim() - len(inner)
        v.ptr[i] = t.data_ptr()
        v.ld[i] = t.stride(nlead - 1) if nlead > 0 else (c if i < 4 else 4 * c)
    return v, keep


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _arr5(ts):
    a = PtrArray5()
    for i in range(5):
        a[i] = ts[i].data_ptr() if (ts is not None and ts[i] is not None) else 0
    return a


def split_packed(t, c):
    """The reference's 5-tuple as zero-copy views of a packed [B,T,8c] tensor."""
    lead = t.shape[:-1]
    return (t[..., 0:c], t[..., c:2 * c], t[..., 2 * c:3 * c], t[..., 3 * c:4 * c],
            t[..., 4 * c:].unflatten(-1, (2, 2 * c)))


# ------------------------------------------------------------------------------------------ launches
def _sample_scale(sample_scale, rows_per_sample, M, ref, what):
    """(sample_scale, rows_per_sample) as every *_skip entry point takes them, for the launcher `what` over M rows of `ref`:
    (None, 0) without a mask; a mask is one float32 factor per sample of rows_per_sample consecutive rows, contiguous, on the
    operands' device (attention: M = B samples of one row).  Anything else is a ValueError here, before any launch; whether
    rows_per_sample is positive and divides M is the library's check (OCTIC_ESHAPE)."""
    if sample_scale is None:
        return None, 0
    rps = int(rows_per_sample)
    if (sample_scale.dtype != torch.float32 or sample_scale.device != ref.device or not sample_scale.is_contiguous()
            or (rps > 0 and M % rps == 0 and sample_scale.numel() != M // rps)):
        raise ValueError(f"{what}: sample_scale must be a contiguous float32 tensor of M / rows_per_sample entries on the "
                         "operands' device")
    return sample_scale, rps


def gelu_fwd(xv, yv, M, c, dtype, ref, sample_scale=None, rows_per_sample=0):
    """sample_scale / rows_per_sample: the stochastic-depth factor of the branch (octic_gelu_d8_fwd_skip) - input rows of a
    sample whose factor is 0 are not read, its output rows are +0."""
    ss, rps = _sample_scale(sample_scale, rows_per_sample, M, ref, "gelu_fwd")
    t = KERNEL_TIMER.start()
    check(lib().octic_gelu_d8_fwd_skip(ctypes.byref(xv), ctypes.byref(yv), M, c, dt_code(dtype), _p(ss), rps, _stream(ref)))
    # (bytes stay the full batch's with a sample_scale: the host does not know the kept count without a sync)
    KERNEL_TIMER.stop(t, f"gelu_fwd_kernel<{_DTN[dtype]}>", 2 * M * 8 * c * ref.element_size())


def gelu_bwd(gv, xv, ov, M, c, dtype, ref, sample_scale=None, rows_per_sample=0):
    """sample_scale / rows_per_sample: as in gelu_fwd (octic_gelu_d8_bwd_skip: neither g nor x is read for a dropped sample)."""
    ss, rps = _sample_scale(sample_scale, rows_per_sample, M, ref, "gelu_bwd")
    t = KERNEL_TIMER.start()
    check(lib().octic_gelu_d8_bwd_skip(ctypes.byref(gv), ctypes.byref(xv), ctypes.byref(ov), M, c, dt_code(dtype), _p(ss), rps,
                                       _stream(ref)))
    KERNEL_TIMER.stop(t, f"gelu_bwd_kernel<{_DTN[dtype]}>", 3 * M * 8 * c * ref.element_size())


def layernorm_fwd(x, alpha5, beta, eps, out_dtype, c, want_stats=True):
    """x: packed f32 [..., 8c] -> (y packed out_dtype, stats [M,8] f32)."""
    M = x.numel() // (8 * c)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    stats = torch.empty((M, 8), dtype=torch.float32, device=x.device) if want_stats else None
    xv, yv = pview(x, c), pview(y, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_layernorm_d8_fwd(ctypes.byref(xv), ctypes.byref(yv), _arr5(alpha5), _p(beta), _p(stats), M, c,
                                       float(eps), dt_code(out_dtype), _stream(x)))
    KERNEL_TIMER.stop(t, f"ln_fwd_kernel<{_DTN[out_dtype]}>", M * 8 * c * (4 + y.element_size()))
    return y, stats


def layernorm_bwd(g, x, stats, alpha5, dres, c, want_param_grads=True, sample_scale=None, rows_per_sample=0):
    """Returns (dx f32 packed, dalpha5 or None, dbeta or None).  dx = dres + LN'(g).
    sample_scale / rows_per_sample: the factor of the branch this norm opens, a promise that the rows of g are zero where it
    is 0 (octic_layernorm_d8_bwd_skip: those rows of g, x and stats stay unread); a malformed mask is a ValueError."""
    M = x.numel() // (8 * c)
    ss, srps = _sample_scale(sample_scale, rows_per_sample, M, x, "layernorm_bwd")
    dx = torch.empty_like(x)
    nblk = lib().octic_layernorm_d8_bwd_blocks(M)
    partials = torch.empty((nblk, 2, 8 * c), dtype=torch.float32, device=x.device)
    gv, xv, dv = pview(g, c), pview(x, c), pview(dx, c)
    rv = pview(dres, c) if dres is not None else None
    t = KERNEL_TIMER.start()
    check(lib().octic_layernorm_d8_bwd_skip(ctypes.byref(gv), ctypes.byref(xv), _p(stats), _arr5(alpha5),
                                            ctypes.byref(rv) if rv is not None else None, ctypes.byref(dv), _p(partials),
                                            M, c, dt_code(g.dtype), _p(ss), srps, _stream(x)))
    KERNEL_TIMER.stop(t, f"ln_bwd_kernel<{_DTN[g.dtype]}>", M * 8 * c * (g.element_size() + 8 + (4 if dres is not None else 0)))
    if not want_param_grads or alpha5 is None:
        return dx, None, None
    dal = [torch.empty_like(a) for a in alpha5]
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    _ln_finish(partials, nblk, c, dal, dbeta, _stream(x))
    return dx, dal, dbeta


def sample_blocks_ok(full, compact, idx):
    return (full.is_cuda and full.is_contiguous() and compact.is_contiguous() and full.dtype == compact.dtype
            and idx.dtype == torch.int64 and idx.is_cuda and full.dim() >= 2 and full.shape[1:] == compact.shape[1:]
            and (full[0].numel() * full.element_size()) % 16 == 0 and 0 < idx.numel() == compact.shape[0] <= 65535)


def gather_samples(full, idx, out=None):
    """full[idx] for whole samples (leading dimension) on csrc/elementwise.hip sample_blocks_kernel."""
    if out is None:
        out = torch.empty((idx.numel(),) + tuple(full.shape[1:]), dtype=full.dtype, device=full.device)
    check(lib().octic_sample_blocks(_p(full), _p(out), _p(idx), idx.numel(), full[0].numel() * full.element_size(), 0,
                                    _stream(full)))
    return out


def scatter_samples_(full, idx, compact):
    """full[idx] = compact, in place (idx distinct)."""
    check(lib().octic_sample_blocks(_p(compact), _p(full), _p(idx), idx.numel(), full[0].numel() * full.element_size(), 1,
                                    _stream(full)))
    return full


def _ln_finish(partials, nblk, c, dal, dbeta, stream):
    """octic_layernorm_d8_bwd_finish now, or batched at the end of the running backward pass (DEFERRED_FINISHES)."""
    if DEFERRED_FINISHES.enabled and _in_backward():
        DEFERRED_FINISHES.add_ln(partials, nblk, c, dal, dbeta, stream)
        return
    check(lib().octic_layernorm_d8_bwd_finish(_p(partials), nblk, c, _arr5(dal), _p(dbeta), stream))


def layernorm_bwd_cast_ok(g, x, c):
    """Shapes of octic_layernorm_d8_bwd_cast: bf16 cotangent, one packed tensor, c = 32 ... 160 in steps of 32."""
    return g.dtype == torch.bfloat16 and x.dtype == torch.float32 and c % 32 == 0 and c <= 160


def layernorm_bwd_cast(g, x, stats, alpha5, dres, c, rs, rps, want_param_grads=True, sample_scale=None, rows_per_sample=0,
                       inplace=False):
    """layernorm_bwd that also returns bf16(rs[row // rps] * dx): (dx, dalpha5, dbeta, gcast).  sample_scale / rows_per_sample:
    as in layernorm_bwd (the factor of the branch this norm opens; rs is that of the branch that ends in front of it).
    inplace (needs the mask and a contiguous f32 dres the caller owns): dres is updated in place and returned as dx
    (octic_layernorm_d8_bwd_cast_inplace: the rows of a dropped sample are not written, and not read where rs is 0)."""
    M = x.numel() // (8 * c)
    ss, srps = _sample_scale(sample_scale, rows_per_sample, M, x, "layernorm_bwd_cast")
    if inplace:
        if ss is None or dres is None or dres.dtype != torch.float32 or not dres.is_contiguous() or dres.numel() != x.numel():
            raise ValueError("layernorm_bwd_cast(inplace=True) needs a sample mask and a contiguous float32 dres of x's size")
        dx = dres
    else:
        dx = torch.empty_like(x)
    gc = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    nblk = lib().octic_layernorm_d8_bwd_blocks(M)
    partials = torch.empty((nblk, 2, 8 * c), dtype=torch.float32, device=x.device)
    gv, xv, dv = pview(g, c), pview(x, c), pview(dx, c)
    rv = pview(dres, c) if dres is not None else None
    t = KERNEL_TIMER.start()
    if inplace:
        check(lib().octic_layernorm_d8_bwd_cast_inplace(ctypes.byref(gv), ctypes.byref(xv), _p(stats), _arr5(alpha5),
                                                        ctypes.byref(dv), _p(partials), M, c, _p(rs), int(rps), _p(gc), _p(ss),
                                                        srps, _stream(x)))
    else:
        check(lib().octic_layernorm_d8_bwd_cast_skip(ctypes.byref(gv), ctypes.byref(xv), _p(stats), _arr5(alpha5),
                                                     ctypes.byref(rv) if rv is not None else None, ctypes.byref(dv),
                                                     _p(partials), M, c, _p(rs), int(rps), _p(gc), _p(ss), srps, _stream(x)))
    KERNEL_TIMER.stop(t, "ln_bwd_kernel<bf16>", M * 8 * c * (2 + 8 + (4 if dres is not None else 0) + 2))
    if not want_param_grads or alpha5 is None:
        return dx, None, None, gc
    dal = [torch.empty_like(a) for a in alpha5]
    dbeta = torch.empty(c, dtype=torch.float32, device=x.device)
    _ln_finish(partials, nblk, c, dal, dbeta, _stream(x))
    return dx, dal, dbeta, gc


_DW_WS = {}


def dense_gemm_ok(rows, N, K):
    """Shapes csrc/dense_gemm.hip takes (y [rows,N] = x [rows,K] W^T; 32-bit buffer offsets: it refuses larger operands)."""
    return K % 64 == 0 and K >= 128 and N % 64 == 0 and N >= 128 and rows * max(N, K) * 2 < 2 ** 31


# Routing policy of this side, stricter than the kernel's 1024-tile limit: the wide TN tiles run only where N x K is at most
# this many 256 x 256 blocks (larger weight gradients stay with the framework's GEMM).
DENSE_WGRAD_MAX_BLOCKS = 256


@torch.compiler.assume_constant_result
def _dense_wgrad_query(M, N0, N1, K, ld_max):
    return _lib.plan("octic_dense_wgrad_plan", M, N0, N1, K, ld_max)


def _dense_wgrad_plan(M, N0, N1, K, ld_max):
    """octic_dense_wgrad_plan's answer, or None for a refusal.  vit._mlp traces through dense_wgrad_ok under torch.compile: the
    tracer keeps the query's answer as a constant instead of tracing into ctypes, and a symbolic row count is pinned to its value
    (operator.index) - the plan is per shape."""
    return _dense_wgrad_query(operator.index(M), N0, N1, K, ld_max)


def dense_wgrad_ok(M, N, K, ld_max=0):
    """The library's TN launcher takes the problem (octic_dense_wgrad_plan; ld_max: the largest operand row stride, 0 = not
    known yet) and, on the wide tiles, the routing cap holds."""
    plan = _dense_wgrad_plan(M, N, 0, K, ld_max)
    return plan is not None and (plan[0] == 64 or (N // 256) * (K // 256) <= DENSE_WGRAD_MAX_BLOCKS)


# Where a weight gradient is to be WRITTEN (train.Trainer under DistributedDataParallel, one micro-batch): parameter address ->
# its bucket view.  A gradient produced inside the bucket is an alias of the view: the reducer recognises it and skips its
# per-tensor copy (reducer.cpp mark_variable_ready_dense).  None = fresh tensors (every other mode).
GRAD_DEST = None


def grad_dest(param, shape):
    """A fresh tensor object aliasing the registered destination of `param`'s gradient, or None."""
    if GRAD_DEST is None or param is None:
        return None
    d = GRAD_DEST.get(param.data_ptr())
    if d is None or param.grad is not None or tuple(d.shape) != tuple(shape) or d.dtype != torch.float32 or not d.is_contiguous():
        return None
    return d.detach()


def grad_written(*params):
    """The launches that write these parameters' gradients into their registered destinations are on the stream: a registry
    that reduces whole buckets as they fill (train.GradReducer) is told; a plain dict (DDP's bucket views) is not."""
    w = getattr(GRAD_DEST, "written", None)
    if w is not None:
        for prm in params:
            if prm is not None:
                w(prm.data_ptr())


def dense_wgrad_tn(dy, x, name=None, out=None, sample_scale=None, rows_per_sample=0):
    """dW[N,K] = dy[M,N]^T @ x[M,K] in f32 on csrc/dense_wgrad.hip (out: write it there).  sample_scale ([M / rows_per_sample]
    f32): the stochastic-depth factor of the branch dy belongs to - a 0 promises that the sample's dy rows are zero, and the
    wide kernel leaves the reduction steps out that only touch such samples (same result; include/octic_hip.h)."""
    _require_cuda(dy)
    M, N = dy.shape
    K = x.shape[1]
    if dy.stride(1) != 1 or x.stride(1) != 1 or x.shape[0] != M:
        raise ValueError("dense_wgrad_tn: operands must be [M,N] / [M,K] row-major")
    ss, rps = _sample_scale(sample_scale, rows_per_sample, M, dy, "dense_wgrad_tn")
    need = int(lib().octic_dense_wgrad_workspace_bytes(M, N, K))
    ws = _DW_WS.get(dy.device)
    if ws is None or ws.numel() < need:          # one workspace per device: launches on a stream are serial
        ws = _DW_WS[dy.device] = torch.zeros(need, dtype=torch.uint8, device=dy.device)
    dw = out if out is not None else torch.empty((N, K), dtype=torch.float32, device=dy.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_wgrad_tn_skip(_p(dy), _p(x), M, N, K, dy.stride(0), x.stride(0), _p(dw), _p(ss), rps, _p(ws),
                                          _stream(dy)))
    KERNEL_TIMER.stop(t, name or f"dense_tn_kernel<{N}x{K}>", 2 * (M * N + M * K) + 4 * N * K, 2.0 * M * N * K)
    return dw


def dense_wgrad_pair_ok(M, N0, N1, K):
    """dense_wgrad_ok for the joint launch of two problems over the same token rows."""
    return (N1 > 0 and _dense_wgrad_plan(M, N0, N1, K, 0) is not None
            and ((N0 + N1) // 256) * (K // 256) <= DENSE_WGRAD_MAX_BLOCKS)


def dense_wgrad_tn_pair(dy0, x0, dy1, x1, dw1=None, dw0=None, sample_scale=None, rows_per_sample=0):
    """(dW0 [N0,K], dW1 [N1,K]) = (dy0^T x0, dy1^T x1) as ONE launch of csrc/dense_wgrad.hip (same M, same K): the qkv and proj
    weight gradients of a standard block.  dw1: write the second result into this (already handed-out) tensor; dw0: a
    registered destination of the first (grad_dest).  sample_scale / rows_per_sample: ONE mask for both problems (qkv and proj
    belong to the same branch), as in dense_wgrad_tn."""
    _require_cuda(dy0)
    M, N0 = dy0.shape
    N1, K = dy1.shape[1], x0.shape[1]
    if not (dy1.shape[0] == M and x0.shape[0] == M and x1.shape == (M, K) and all(t.stride(1) == 1 for t in (dy0, x0, dy1, x1))):
        raise ValueError("dense_wgrad_tn_pair: operands must be [M,N0] / [M,K] / [M,N1] / [M,K] row-major")
    ss, rps = _sample_scale(sample_scale, rows_per_sample, M, dy0, "dense_wgrad_tn_pair")
    need = int(lib().octic_dense_wgrad_pair_workspace_bytes(M, N0, N1, K))
    ws = _DW_WS.get(dy0.device)
    if ws is None or ws.numel() < need:
        ws = _DW_WS[dy0.device] = torch.zeros(need, dtype=torch.uint8, device=dy0.device)
    if dw0 is None:
        dw0 = torch.empty((N0, K), dtype=torch.float32, device=dy0.device)
    if dw1 is None:
        dw1 = torch.empty((N1, K), dtype=torch.float32, device=dy0.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_wgrad_tn_pair_skip(_p(dy0), _p(x0), N0, dy0.stride(0), x0.stride(0), _p(dw0), _p(dy1), _p(x1), N1,
                                               dy1.stride(0), x1.stride(0), _p(dw1), M, K, _p(ss), rps, _p(ws), _stream(dy0)))
    KERNEL_TIMER.stop(t, f"dense_tn_kernel<{N0}+{N1}x{K}>", 2 * M * (N0 + N1 + 2 * K) + 4 * (N0 + N1) * K, 2.0 * M * (N0 + N1) * K)
    return dw0, dw1


def linear_fwd(xv, w5, bias, yv, M, cin, cout, dtype, out_dtype, ref, resid_v=None, rs=None, rps=1, cs5=None, sample_scale=None,
               skip_rps=0, dropped=None, dropped_rps=0):
    """sample_scale / skip_rps (plain launches only): the stochastic-depth factor of the branch, one entry per sample of
    skip_rps rows, where EVERY reader of the output honours the same mask (octic_linear_d8_fwd_skip: the output rows of a
    dropped sample may stay unwritten).  dropped / dropped_rps: the same factor under the other contract
    (octic_linear_d8_fwd_dropped): the input rows of a dropped sample are zero (plain launch, no bias) or rs is that mask (fused);
    every output row is written.  One mask per call.  Timer name, bytes and FLOP stay the full batch's."""
    ss, srps = _sample_scale(sample_scale, skip_rps, M, ref, "linear_fwd")
    dr, drps = _sample_scale(dropped, dropped_rps, M, ref, "linear_fwd")
    if ss is not None and dr is not None:
        raise ValueError("linear_fwd: sample_scale and dropped are two contracts for one mask - pass one of them")
    t = KERNEL_TIMER.start()
    entry = lib().octic_linear_d8_fwd_skip if dr is None else lib().octic_linear_d8_fwd_dropped
    check(entry(ctypes.byref(xv), _arr5(w5), _p(bias), ctypes.byref(yv),
                ctypes.byref(resid_v) if resid_v is not None else None, _p(rs), int(rps),
                _arr5(cs5) if cs5 is not None else None, M, cin, cout, dt_code(dtype),
                dt_code(out_dtype), _p(ss if dr is None else dr), srps if dr is None else drps, _stream(ref)))
    if t is not None:
        es, eo = (2 if dtype == torch.bfloat16 else 4), (2 if out_dtype == torch.bfloat16 else 4)
        nbytes = M * 8 * cin * es + M * 8 * cout * eo * (2 if resid_v is not None else 1) + 8 * cin * cout * es
        fused = int(resid_v is not None or rs is not None or cs5 is not None)
        KERNEL_TIMER.stop(t, linear_kernel_name(cin, cout, dtype, out_dtype, fused, M), nbytes, 24.0 * M * cin * cout)


def linear_kernel_name(cin, cout, dtype, out_dtype, fused, M):
    """Name of the kernel instantiation octic_linear_d8_fwd runs for this call, from the library's plan."""
    kernel, _, fused, _ = _lib.plan("octic_linear_d8_plan", M, cin, cout, dt_code(dtype), dt_code(out_dtype), int(fused))
    if kernel == _lib.LINEAR_WREG:
        return f"linear_d8_wreg_kernel<{_DTN[out_dtype]},{fused}>"
    if kernel == _lib.LINEAR_RING:
        return f"linear_d8_ring_kernel<{_DTN[dtype]},{_DTN[out_dtype]},{fused}>"
    return f"linear_d8_kernel<{_DTN[dtype]},{_DTN[out_dtype]}>"


def linear_wgrad(xv, dyv, M, cin, cout, dtype, ref, w32=None, cs5=None, bias=None, dysum=None, want_bias=False,
                 may_defer=True, wparams=None, sample_scale=None, rows_per_sample=0):
    """Returns (dw5 [f32], dcs5 or None, dbias or None).  may_defer=False: the caller reads the results at once (e.g. casts
    them for non-f32 master weights), so the slab reduction must not be postponed to the end of the backward pass.
    sample_scale / rows_per_sample (functional.linear_wgrad_skip_scale): the stochastic-depth factor of the branch, zero for
    the samples whose dy rows are all zero; the ring kernel then walks the live steps only (octic_linear_d8_wgrad_skip).  The
    booked name, bytes and FLOP stay those of the full batch."""
    L = lib()
    dev = ref.device
    kernel, tile, splits, _ = _lib.plan("octic_linear_d8_wgrad_plan", M, cin, cout, dt_code(dtype))
    ws = torch.empty(L.octic_linear_d8_wgrad_workspace_bytes(cin, cout, splits) // 4, dtype=torch.float32, device=dev)
    t = KERNEL_TIMER.start()
    if sample_scale is None:
        check(L.octic_linear_d8_wgrad(ctypes.byref(xv), ctypes.byref(dyv), M, cin, cout, dt_code(dtype), _p(ws), splits,
                                      _stream(ref)))
    else:
        check(L.octic_linear_d8_wgrad_skip(ctypes.byref(xv), ctypes.byref(dyv), M, cin, cout, dt_code(dtype), _p(ws), splits,
                                           _p(sample_scale), int(rows_per_sample), _stream(ref)))
    if t is not None:
        es = 2 if dtype == torch.bfloat16 else 4
        name = "wgrad_ring_kernel<bf16>" if kernel == _lib.WGRAD_RING else f"wgrad_kernel<{_DTN[dtype]},{tile // 32}>"
        # slabs: the two-dimensional irrep (half of the 8*cin*cout weights) uses `splits`, the others splits/2
        slab = (splits + (splits + 1) // 2) * 4 * cin * cout * 4
        KERNEL_TIMER.stop(t, name, M * 8 * (cin + cout) * es + slab, 24.0 * M * cin * cout)
    shapes = [(cout, cin)] * 4 + [(2 * cout, 2 * cin)]
    dests = [grad_dest(w, sh) for w, sh in zip(wparams, shapes)] if wparams is not None else [None] * 5
    dw = [d if d is not None else torch.empty(sh, dtype=torch.float32, device=dev) for d, sh in zip(dests, shapes)]
    dcs = None
    if cs5 is not None:
        dcs = [torch.empty(cout, dtype=torch.float32, device=dev) for _ in range(4)]
        dcs.append(torch.empty(2 * cout, dtype=torch.float32, device=dev))
    dbias = torch.empty(cout, dtype=torch.float32, device=dev) if want_bias else None
    landed = [w for w, d in zip(wparams, dests) if d is not None] if wparams is not None else []
    if may_defer and DEFERRED_FINISHES.enabled and DEFERRED_FINISHES.slabs_too and _in_backward():
        DEFERRED_FINISHES.add_wg(ws, splits, cin, cout, w32, cs5, bias, dysum, dw, dcs, dbias, _stream(ref), landed)
        return dw, dcs, dbias
    check(L.octic_linear_d8_wgrad_finish(_p(ws), splits, cin, cout, _arr5(w32) if cs5 is not None else None,
                                         _arr5(cs5) if cs5 is not None else None, _p(bias), _p(dysum), _arr5(dw),
                                         _arr5(dcs) if dcs is not None else None, _p(dbias), _stream(ref)))
    grad_written(*landed)
    return dw, dcs, dbias


def wgrad_has_colsum(cin, cout, dtype):
    """Whether the wgrad launch leaves the A1 column sums behind its slabs (the answer does not depend on the row count)."""
    return bool(_lib.plan("octic_linear_d8_wgrad_plan", 1, cin, cout, dt_code(dtype))[3])


def colsum_a1(dyv, M, c, dtype, ref):
    L = lib()
    nblk = L.octic_colsum_blocks(M)
    partials = torch.empty((nblk, c), dtype=torch.float32, device=ref.device)
    out = torch.empty(c, dtype=torch.float32, device=ref.device)
    check(L.octic_colsum_a1(ctypes.byref(dyv), M, c, dt_code(dtype), _p(partials), _p(out), _stream(ref)))
    return out


def cast_rowscale(x, rs, rps, out_dtype, c):
    M = x.numel() // (8 * c)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    xv, yv = pview(x, c), pview(y, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_cast_rowscale(ctypes.byref(xv), ctypes.byref(yv), _p(rs), int(rps), M, c, dt_code(out_dtype),
                                    _stream(x)))
    KERNEL_TIMER.stop(t, f"cast_rowscale_kernel<{_DTN[out_dtype]}>", M * 8 * c * (4 + y.element_size()))
    return y


def _arr3(ts):
    a = (ctypes.c_void_p * 3)()
    for i in range(3):
        a[i] = ts[i].data_ptr() if i < len(ts) else 0
    return a


def pack_heads(x, B, T, H, c, n_s):
    """x packed [B,T,n_s*8c] -> n_s separate tensors [B,H,T,8c/H]"""
    outs = [torch.empty((B, H, T, 8 * c // H), dtype=x.dtype, device=x.device) for _ in range(n_s)]
    xv = pview(x, n_s * c)
    t = KERNEL_TIMER.start()
    check(lib().octic_attn_pack_heads(ctypes.byref(xv), _arr3(outs), B, T, H, c, n_s, dt_code(x.dtype), _stream(x)))
    KERNEL_TIMER.stop(t, f"heads_permute_kernel<{_DTN[x.dtype]},pack>", 2 * x.numel() * x.element_size())
    return outs


def unpack_heads(heads, B, T, H, c):
    """list of n_s tensors [B,H,T,8c/H] -> packed [B,T,n_s*8c]"""
    heads = [h if h.is_contiguous() else h.contiguous() for h in heads]
    n_s = len(heads)
    y = torch.empty((B, T, n_s * 8 * c), dtype=heads[0].dtype, device=heads[0].device)
    yv = pview(y, n_s * c)
    t = KERNEL_TIMER.start()
    check(lib().octic_attn_unpack_heads(_arr3(heads), ctypes.byref(yv), B, T, H, c, n_s, dt_code(y.dtype), _stream(y)))
    KERNEL_TIMER.stop(t, f"heads_permute_kernel<{_DTN[y.dtype]},unpack>", 2 * y.numel() * y.element_size())
    return y


def linear_prep(w5, cs5, cin, cout, dtype, want_wb=True):
    """One launch: (wb list of 5 views | None, wt list of 5 views) in `dtype` (see octic_linear_d8_prep)."""
    dev = w5[0].device
    n = 8 * cin * cout
    wb = torch.empty(n, dtype=dtype, device=dev) if want_wb else None
    wt = torch.empty(n, dtype=dtype, device=dev)
    check(lib().octic_linear_d8_prep(_arr5(w5), _arr5(cs5) if cs5 is not None else None, cin, cout, _p(wb), _p(wt),
                                     dt_code(dtype), _stream(w5[0])))
    return prep_views(wb, cin, cout, False), prep_views(wt, cin, cout, True)


def prep_views(flat, cin, cout, transposed):
    """The five per-irrep matrices inside a flat prepared-weight buffer ([cout,cin] or, transposed, [cin,cout])."""
    if flat is None:
        return None
    small = cin * cout
    out = [flat[i * small:(i + 1) * small].view((cin, cout) if transposed else (cout, cin)) for i in range(4)]
    out.append(flat[4 * small:].view((2 * cin, 2 * cout) if transposed else (2 * cout, 2 * cin)))
    return out


def attn_fwd(q, k, v, scale, out=None, sample_scale=None):
    """q,k,v: [B,H,T,hd] bf16 or float32 views with a common stride set (last dim contiguous) -> (o [B,H,T,hd],
    lse [B,H,T]); out: an optional [B,H,T,hd] view (last dim contiguous, 16-byte rows) that receives o.  float32
    operands run octic_attn_fwd_f32 (csrc/attn_f32.hip).  sample_scale ([B] f32, bf16 operands only): the factor the caller
    multiplies each sample's branch output with - a kernel may skip the samples whose factor is 0 and write zeros
    (include/octic_hip.h, octic_attn_fwd_skip)."""
    B, H, T, hd = q.shape
    st = q.stride()
    if st[3] != 1 or k.stride() != st or v.stride() != st:
        raise ValueError("attn_fwd: q, k, v must share strides and be contiguous in the last dim")
    if out is not None and (out.shape != q.shape or out.dtype != q.dtype or out.device != q.device or out.stride(3) != 1):
        raise ValueError("attn_fwd: out must match q in shape, dtype and device and be contiguous in the last dim")
    o = out if out is not None else torch.empty((B, H, T, hd), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    f32 = q.dtype == torch.float32
    t = KERNEL_TIMER.start()
    if f32:
        check(lib().octic_attn_fwd_f32(_p(q), _p(k), _p(v), _p(o), _p(lse), B, H, T, hd, st[0], st[1], st[2],
                                       o.stride(0), o.stride(1), o.stride(2), float(scale), _stream(q)))
    else:
        ss, _ = _sample_scale(sample_scale, 1, B, q, "attn_fwd")
        check(lib().octic_attn_fwd_skip(_p(q), _p(k), _p(v), _p(o), _p(lse), B, H, T, hd, st[0], st[1], st[2],
                                        o.stride(0), o.stride(1), o.stride(2), float(scale), _p(ss), _stream(q)))
    # (bytes and FLOP stay the full batch's with a sample_scale: the host does not know the kept count without a sync)
    KERNEL_TIMER.stop(t, _attn_fwd_name(T, hd, dt_code(q.dtype), (st[2], o.stride(2), 0)), 4 * q.numel() * q.element_size(),
                      4.0 * B * H * T * T * hd)
    return o, lse


ATTN_MAX_T = 16384      # octic_attn_*: longest sequence of the streaming kernels


def attn_supported(T, hd, dtype):
    """Shapes the HIP attention core handles (others keep torch SDPA): bf16, 0 < T <= 16384, hd % 16 == 0, hd <= 128."""
    return dtype == torch.bfloat16 and 0 < T <= ATTN_MAX_T and hd % 16 == 0 and 0 < hd <= 128


ATTN_F32_ROWS = 128     # csrc/attn_f32.hip, kF32Rows: own rows (queries / keys) of a workgroup
ATTN_F32_BLK = 32       # csrc/attn_f32.hip, kF32Blk: streamed rows per LDS block


def attn_f32_supported(T, hd, dtype):
    """Shapes of octic_attn_{fwd,bwd}_f32 (exact-f32 MFMA, one streaming design): float32, 0 < T <= 16384, hd % 16 == 0,
    hd <= 128.  attn_supported / attn_packed_ok stay bf16-only predicates."""
    return dtype == torch.float32 and 0 < T <= ATTN_MAX_T and hd % 16 == 0 and 0 < hd <= 128


def attn_streams(T, hd, backward=False):
    """True where the entry points run the streaming kernels (csrc/attn_stream.hip: K / V through LDS in blocks): what
    octic_attn_plan says for contiguous bf16 heads under the current route overrides."""
    plan = _lib.attn_plan(T, hd)
    return plan[2] == _lib.ATTN_BWD_STREAM if backward else plan[0] == _lib.ATTN_FWD_STREAM


_ATTN_FWD_NAMES = {_lib.ATTN_FWD_STREAM: "attn_fwd_stream_kernel", _lib.ATTN_FWD_F32: "attn_f32_fwd_kernel"}


def _attn_fwd_name(T, hd, dtype=_lib.BF16, ld=(0, 0, 0)):
    """Timer name of the forward launch octic_attn_plan names; ld = token strides of q/k/v, o, gradients (0: hd)."""
    return _ATTN_FWD_NAMES.get(_lib.attn_plan(T, hd, dtype, *ld)[0], "attn_fwd_kernel")


# Single-pass attention backward (csrc/attn80_bwd.hip: P and dS computed once, 10 T^2 hd FLOP) where octic_attn_plan has it;
# False = the dq + dkv pair (14 T^2 hd) for every shape (bench --no-fused-attn-bwd)
ATTN_BWD_FUSED = True


def _attn_bwd_phases(T, hd, dtype=_lib.BF16, ld=(0, 0, 0)):
    """(phase, timer name, algorithmic bytes per element of q, flops per B H T^2 hd) of the backward launches: one phase-3
    call exactly where ATTN_BWD_FUSED is on and octic_attn_plan says SINGLE, else phase 1 (dq: 3 products) and phase 2
    (dk, dv: 4 products), named after the plan."""
    bwd = _lib.attn_plan(T, hd, dtype, *ld)[2]
    if ATTN_BWD_FUSED and bwd == _lib.ATTN_BWD_SINGLE:
        return ((3, "attn_bwd_kernel", 8, 10.0),)         # reads q k v o dO, writes dq dk dv
    pre = "attn_f32" if bwd == _lib.ATTN_BWD_F32 else "attn_bwd"
    suf = "_stream_kernel" if bwd == _lib.ATTN_BWD_STREAM else "_kernel"
    return ((1, pre + "_dq" + suf, 6, 6.0), (2, pre + "_dkv" + suf, 6, 8.0))


def attn_skips_dropped(B, T, hd, dtype=_lib.BF16, ld=(0, 0, 0)):
    """True where BOTH attention launches of a training step - the forward and whatever _attn_bwd_phases runs - SKIP a sample
    whose sample_scale is 0: they read none of its q / k / v / dO rows (octic_attn_skip_plan, under the current route overrides).
    Only then may the GEMMs around the softmax core (qkv's forward, proj's input gradient) leave those rows unwritten: a kernel
    that computes the sample would carry whatever the rows hold into the stream as 0 x NaN."""
    answer = _lib.plan("octic_attn_skip_plan", dtype, T, hd, *ld)
    if answer is None:
        return False
    fwd_max_b, single, pair, _ = answer
    bwd = single if _attn_bwd_phases(T, hd, dtype, ld)[0][0] == 3 else pair
    return bool(0 < B <= fwd_max_b and bwd)


def attn_bwd(q, k, v, o, dout, lse, scale, dq, dk, dv, sample_scale=None):
    """All tensors are [B,H,T,hd] views (bf16, or all float32: octic_attn_bwd_f32); q/k/v share strides, o/dout share
    strides, dq/dk/dv share strides.  sample_scale: as in attn_fwd (a skipped sample gets zeros in dq, dk, dv)."""
    B, H, T, hd = q.shape
    st, so, sg = q.stride(), o.stride(), dq.stride()
    if k.stride() != st or v.stride() != st or dout.stride() != so or dk.stride() != sg or dv.stride() != sg:
        raise ValueError("attn_bwd: stride sets differ")
    delta = torch.empty((B, H, T), dtype=torch.float32, device=q.device)
    f32 = q.dtype == torch.float32
    phases = _attn_bwd_phases(T, hd, dt_code(q.dtype), (st[2], so[2], sg[2]))
    ss = None if f32 else _sample_scale(sample_scale, 1, B, q, "attn_bwd")[0]
    for phase, name, nbytes, flops in phases:
        t = KERNEL_TIMER.start()
        args = (_p(q), _p(k), _p(v), _p(o), _p(dout), _p(lse), _p(delta), _p(dq), _p(dk), _p(dv), B, H,
                T, hd, st[0], st[1], st[2], so[0], so[1], so[2], sg[0], sg[1], sg[2], float(scale), phase)
        if f32:
            check(lib().octic_attn_bwd_f32(*args, _stream(q)))
        else:
            check(lib().octic_attn_bwd_skip(*args, _p(ss), _stream(q)))
        KERNEL_TIMER.stop(t, name, nbytes * q.numel() * q.element_size(), flops * B * H * T * T * hd)


def attn_packed_ok(T, c, H, dtype):
    """Shapes of octic_attn_{fwd,bwd}_packed: bf16, head_dim 80 (c = 10 H: ViT-H/14) or 64 (c = 8 H: ViT-L/16), T <= 16384."""
    return dtype == torch.bfloat16 and c in (10 * H, 8 * H) and attn_supported(T, 8 * (c // H), dtype)


def attn_fwd_packed(qkv, H, c, scale, out=None, sample_scale=None):
    """qkv packed [B,T,3*8c] bf16 -> (o packed [B,T,8c], lse [B,H,T]); no head pack / unpack copies.  sample_scale: as in
    attn_fwd."""
    B, T = qkv.shape[0], qkv.shape[1]
    o = out if out is not None else torch.empty((B, T, 8 * c), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device)
    ss, _ = _sample_scale(sample_scale, 1, B, qkv, "attn_fwd_packed")
    t = KERNEL_TIMER.start()
    check(lib().octic_attn_fwd_packed_skip(_p(qkv), _p(o), _p(lse), B, H, T, c, qkv.stride(1), o.stride(1), float(scale),
                                           _p(ss), _stream(qkv)))
    KERNEL_TIMER.stop(t, _attn_fwd_name(T, 8 * (c // H), ld=(qkv.stride(1), o.stride(1), 0)), 4 * B * T * 8 * c * 2,
                      4.0 * B * T * T * 8 * c)
    return o, lse


def attn_bwd_packed(qkv, o, dout, lse, H, c, scale, out=None, sample_scale=None):
    """-> dqkv packed [B,T,3*8c] (dq | dk | dv in the layout of qkv).  sample_scale: as in attn_bwd."""
    B, T = qkv.shape[0], qkv.shape[1]
    dqkv = out if out is not None else torch.empty_like(qkv)
    delta = torch.empty((B, H, T), dtype=torch.float32, device=qkv.device)
    ss, _ = _sample_scale(sample_scale, 1, B, qkv, "attn_bwd_packed")
    for phase, name, nbytes, flops in _attn_bwd_phases(T, 8 * (c // H), ld=(qkv.stride(1), o.stride(1), dqkv.stride(1))):
        t = KERNEL_TIMER.start()
        check(lib().octic_attn_bwd_packed_skip(_p(qkv), _p(o), _p(dout), _p(lse), _p(delta), _p(dqkv), B, H, T, c,
                                               qkv.stride(1), o.stride(1), dqkv.stride(1), float(scale), phase, _p(ss),
                                               _stream(qkv)))
        KERNEL_TIMER.stop(t, name, nbytes * B * T * 8 * c * 2, flops * B * T * T * 8 * c)
    return dqkv


def handoff_cat_fwd(x, c, out_dtype):
    M = x.numel() // (8 * c)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    xv = pview(x, c)
    check(lib().octic_handoff_cat_fwd(ctypes.byref(xv), _p(y), M, c, dt_code(out_dtype), _stream(x)))
    return y


def handoff_cat_bwd(dd, c):
    dd = dd.contiguous().float()
    M = dd.numel() // (8 * c)
    dx = torch.empty_like(dd)
    dv = pview(dx, c)
    check(lib().octic_handoff_cat_bwd(_p(dd), ctypes.byref(dv), M, c, _stream(dd)))
    return dx


def power_spectrum_fwd(x, c, out_dtype):
    M = x.numel() // (8 * c)
    y = torch.empty(x.shape[:-1] + (6 * c,), dtype=out_dtype, device=x.device)
    xv = pview(x, c)
    check(lib().octic_power_spectrum_fwd(ctypes.byref(xv), _p(y), M, c, dt_code(out_dtype), _stream(x)))
    return y


def power_spectrum_bwd(dd, x, c):
    dd = dd.contiguous().float()
    M = x.numel() // (8 * c)
    dx = torch.empty_like(x)
    xv, dv = pview(x, c), pview(dx, c)
    check(lib().octic_power_spectrum_bwd(_p(dd), ctypes.byref(xv), ctypes.byref(dv), M, c, _stream(x)))
    return dx


def im2col(img, p, Kpad, dtype):
    B, Cin, Hh, Ww = img.shape
    img = img.contiguous().float()
    rows = B * (Hh // p) * (Ww // p)
    out = torch.empty((rows, Kpad), dtype=dtype, device=img.device)
    check(lib().octic_im2col_patches(_p(img), _p(out), B, Cin, Hh, Ww, p, Kpad, dt_code(dtype), _stream(img)))
    return out


def lift_gemm(patches, w, bias_full, pos, out, B, n_patches, tok0, Kpad, D):
    check(lib().octic_lift_gemm(_p(patches), _p(w), _p(bias_full), _p(pos), _p(out), B, n_patches, tok0, Kpad, D,
                                dt_code(patches.dtype), _stream(patches)))


def lift_wgrad(patches, dout, Kpad, D):
    L = lib()
    rows = patches.shape[0]
    splits = max(1, min(16, rows // 512))
    ws = torch.empty(L.octic_lift_wgrad_workspace_bytes(Kpad, D, splits) // 4, dtype=torch.float32, device=patches.device)
    dw = torch.empty((D, Kpad), dtype=torch.float32, device=patches.device)
    check(L.octic_lift_wgrad(_p(patches), _p(dout), _p(dw), _p(ws), splits, rows, Kpad, D, dt_code(patches.dtype),
                             _stream(patches)))
    return dw


# ------------------------------------------------------------------------------------------ standard half
class _FinishJob(ctypes.Structure):
    _fields_ = [("partials", ctypes.c_void_p), ("out0", ctypes.c_void_p), ("out1", ctypes.c_void_p),
                ("scale1", ctypes.c_void_p), ("nblocks", ctypes.c_int), ("d", ctypes.c_int)]


class _LnFinishJob(ctypes.Structure):
    _fields_ = [("partials", ctypes.c_void_p), ("dalpha", ctypes.c_void_p * 5), ("dbeta", ctypes.c_void_p),
                ("nblk", ctypes.c_int), ("c", ctypes.c_int)]


class _WgFinishJob(ctypes.Structure):
    _fields_ = [("workspace", ctypes.c_void_p), ("w32", ctypes.c_void_p * 5), ("cs", ctypes.c_void_p * 5),
                ("bias", ctypes.c_void_p), ("dysum", ctypes.c_void_p), ("dw", ctypes.c_void_p * 5),
                ("dcs", ctypes.c_void_p * 5), ("dbias", ctypes.c_void_p),
                ("splits", ctypes.c_int), ("cin", ctypes.c_int), ("cout", ctypes.c_int), ("has_cs", ctypes.c_int)]


class _DeferredFinishes:
    """Parameter-gradient slab reductions (octic_dense_finish) postponed to the end of the running backward pass and issued
    as ONE batched launch (octic_dense_finish_batch: same summation order, bit-identical results).  Only the caller knows that
    nothing reads those gradients earlier (no gradient accumulation into an existing .grad - which includes a parameter used
    twice in one pass: autograd adds its second gradient to the first at once -, no DDP bucket hooks, no tensor hooks):
    `train.Trainer` switches this on for its single-GPU, single-micro-batch step of a model whose parameters each enter the
    graph once; the default is immediate launches."""

    def __init__(self):
        self.enabled = False
        self.slabs_too = True   # also postpone the octic weight-gradient slab reductions (their 50 MB slabs stay allocated
                                # until the end of the pass: off when the launch shapes vary from step to step)
        self.jobs = []          # (partials, nblk, d, out0_ptr, out1_ptr, scale1, keep-alive tensors, stream)
        self.ln_jobs = []       # (partials, nblk, c, [5 dalpha ptrs], dbeta_ptr, keep-alive storages, stream)
        self.wg_jobs = []       # (filled _WgFinishJob, keep-alive tensors / storages, stream)
        self.pairs = []         # functional.WgradPair objects holding a postponed weight gradient (see there)
        self.allow_pairs = True  # False: weight gradients are never postponed (they are read early: DDP's reducer hooks)
        self.armed = False

    def add_pair(self, pair):
        self.pairs.append(pair)
        if not self.armed:
            self.armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def add(self, partials, nblk, d, out0_ptr, out1_ptr, scale1, keep, stream):
        self.jobs.append((partials, nblk, d, out0_ptr, out1_ptr, scale1, keep, stream))
        if not self.armed:
            self.armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def add_ln(self, partials, nblk, c, dal, dbeta, stream):
        keep = tuple(t.untyped_storage() for t in list(dal) + [dbeta] if t is not None)
        self.ln_jobs.append((partials, nblk, c, [t.data_ptr() if t is not None else None for t in dal],
                             dbeta.data_ptr() if dbeta is not None else None, keep, stream))
        if not self.armed:
            self.armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def add_wg(self, ws, splits, cin, cout, w32, cs5, bias, dysum, dw, dcs, dbias, stream, landed=()):
        j = _WgFinishJob()
        j.workspace = ws.data_ptr()
        j.has_cs = 1 if cs5 is not None else 0
        for k in range(5):
            j.w32[k] = w32[k].data_ptr() if cs5 is not None else None
            j.cs[k] = cs5[k].data_ptr() if cs5 is not None else None
            j.dw[k] = dw[k].data_ptr()
            j.dcs[k] = dcs[k].data_ptr() if dcs is not None else None
        j.bias = bias.data_ptr() if bias is not None else None
        j.dysum = dysum.data_ptr() if dysum is not None else None
        j.dbias = dbias.data_ptr() if dbias is not None else None
        j.splits, j.cin, j.cout = splits, cin, cout
        outs = list(dw) + (list(dcs) if dcs is not None else []) + ([dbias] if dbias is not None else [])
        keep = (ws, w32 if cs5 is not None else None, cs5, bias, dysum, tuple(t.untyped_storage() for t in outs))
        self.wg_jobs.append((j, keep, stream, tuple(landed)))
        if not self.armed:
            self.armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def flush(self):
        pairs, self.pairs = self.pairs, []
        for pr in pairs:                                # a postponed weight gradient whose partner never came: on its own now
            pr.flush()
        jobs, self.jobs, self.armed = self.jobs, [], False
        ln_jobs, self.ln_jobs = self.ln_jobs, []
        wg_jobs, self.wg_jobs = self.wg_jobs, []
        if wg_jobs:
            arr = (_WgFinishJob * len(wg_jobs))(*[j[0] for j in wg_jobs])
            t = KERNEL_TIMER.start()
            check(lib().octic_linear_d8_wgrad_finish_batch(ctypes.cast(arr, ctypes.c_void_p), len(wg_jobs), wg_jobs[0][2]))
            KERNEL_TIMER.stop(t, "wgrad_finish_batch_kernel", 0)
            for j in wg_jobs:                           # gradients that went into registered destinations are there now
                grad_written(*j[3])
        if ln_jobs:
            arr = (_LnFinishJob * len(ln_jobs))()
            for i, (partials, nblk, c, dal, dbeta, _keep, _s) in enumerate(ln_jobs):
                arr[i].partials = partials.data_ptr()
                for k in range(5):
                    arr[i].dalpha[k] = dal[k]
                arr[i].dbeta = dbeta
                arr[i].nblk, arr[i].c = nblk, c
            t = KERNEL_TIMER.start()
            check(lib().octic_layernorm_d8_bwd_finish_batch(ctypes.cast(arr, ctypes.c_void_p), len(ln_jobs), ln_jobs[0][6]))
            KERNEL_TIMER.stop(t, "ln_bwd_finish_batch_kernel", sum(j[1] * 2 * 8 * j[2] * 4 for j in ln_jobs))
        if not jobs:
            return
        arr = (_FinishJob * len(jobs))()
        for i, (partials, nblk, d, o0, o1, sc, _keep, _s) in enumerate(jobs):
            arr[i].partials = partials.data_ptr()
            arr[i].out0 = o0
            arr[i].out1 = o1
            arr[i].scale1 = sc.data_ptr() if sc is not None else None
            arr[i].nblocks = nblk
            arr[i].d = d
        t = KERNEL_TIMER.start()
        check(lib().octic_dense_finish_batch(ctypes.cast(arr, ctypes.c_void_p), len(jobs), jobs[0][7]))
        KERNEL_TIMER.stop(t, "dense_finish_batch_kernel", sum(j[1] * 2 * j[2] * 4 for j in jobs))


DEFERRED_FINISHES = _DeferredFinishes()


def _in_backward():
    try:
        return torch._C._current_graph_task_id() != -1
    except Exception:
        return False


def _finish(partials, nblk, d, out0, out1, scale1, stream, out1_ptr=None):
    """out0[j] = sum_b partials[b][0][j], out1[j] = scale1[j] * sum_b partials[b][1][j] - now, or (see _DeferredFinishes) at the
    end of the running backward pass.  out1_ptr: raw address for an out1 that is the second half of out0's storage."""
    o0 = out0.data_ptr() if out0 is not None else None
    o1 = out1_ptr if out1_ptr is not None else (out1.data_ptr() if out1 is not None else None)
    if DEFERRED_FINISHES.enabled and _in_backward():
        # keep the outputs' STORAGE alive, not the tensors: a second reference to the tensor would make AccumulateGrad clone
        # the (not yet written) gradient instead of adopting it
        keep = tuple(t.untyped_storage() for t in (out0, out1) if t is not None)
        DEFERRED_FINISHES.add(partials, nblk, d, o0, o1, scale1, keep, stream)
        return
    check(lib().octic_dense_finish(_p(partials), nblk, d, ctypes.c_void_p(o0) if o0 else None,
                                   ctypes.c_void_p(o1) if o1 else None, _p(scale1), stream))


def dense_layernorm_fwd(x, w, b, eps, out_dtype):
    """x: f32 [..., d] contiguous -> (y out_dtype, stats [rows, 2] f32 = (mean, rstd))."""
    _require_cuda(x)
    d = x.shape[-1]
    rows = x.numel() // d
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_layernorm_fwd(_p(x), _p(y), dt_code(out_dtype), _p(w), _p(b), _p(stats), rows, d, float(eps),
                                          _stream(x)))
    KERNEL_TIMER.stop(t, f"dense_ln_fwd_kernel<{_DTN[out_dtype]}>", rows * d * (4 + y.element_size()))
    return y, stats


def _check_rowmap(rowmap, rows):
    if rowmap.dtype != torch.int32 or not rowmap.is_contiguous() or rowmap.numel() != rows:
        raise ValueError("row map: a contiguous int32 tensor with one entry per compact row")


def dense_layernorm_fwd_rows(x, rowmap, w, b, eps, out_dtype):
    """LayerNorm of rows rowmap[r] of the f32 stream x [..., d] -> (y [1, rows, d] out_dtype, stats, xa = those rows, compact)."""
    _require_cuda(x)
    d = x.shape[-1]
    rows = rowmap.numel()
    _check_rowmap(rowmap, rows)
    y = torch.empty((1, rows, d), dtype=out_dtype, device=x.device)
    xa = torch.empty((1, rows, d), dtype=torch.float32, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_layernorm_fwd_rows(_p(x), _p(y), dt_code(out_dtype), _p(w), _p(b), _p(stats), rows, d, float(eps),
                                               _p(rowmap), _p(xa), _stream(x)))
    KERNEL_TIMER.stop(t, f"dense_ln_fwd_kernel<{_DTN[out_dtype]},rows>", rows * d * (8 + y.element_size()))
    return y, stats, xa


def dense_layernorm_bwd_rows_(gy, xa, w, stats, g, rowmap, want_param_grads=True):
    """In place on the stream's cotangent g: g[rowmap[r]] = LN'(gy[r]; xa[r]) + g[rowmap[r]].  Returns (dw, db)."""
    d = xa.shape[-1]
    rows = rowmap.numel()
    _check_rowmap(rowmap, rows)
    nblk = lib().octic_dense_blocks(rows)
    partials = torch.empty((nblk, 2, d), dtype=torch.float32, device=xa.device) if want_param_grads else None
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_layernorm_bwd_rows(_p(gy), dt_code(gy.dtype), _p(xa), _p(w), _p(stats), _p(g), _p(g), _p(partials),
                                               rows, d, _p(rowmap), _stream(xa)))
    KERNEL_TIMER.stop(t, f"dense_ln_bwd_kernel<{_DTN[gy.dtype]},rows>", rows * d * (gy.element_size() + 12))
    if not want_param_grads:
        return None, None
    dw = torch.empty(d, dtype=torch.float32, device=xa.device)
    db = torch.empty(d, dtype=torch.float32, device=xa.device)
    _finish(partials, nblk, d, dw, db, None, _stream(xa))
    return dw, db


def dense_resid_layernorm_fwd(x, yb, gamma, rs, rps, w, b, eps, out_dtype, skip_yb=False):
    """xout = x + rs[row // rps] * gamma * yb ; y = LayerNorm(xout) in one row pass -> (xout f32, y out_dtype, stats).
    skip_yb (with rs): the rows of yb whose factor is 0 stay unread (octic_dense_resid_layernorm_fwd_skip)."""
    _require_cuda(x)
    d = x.shape[-1]
    rows = x.numel() // d
    xout = torch.empty_like(x)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    t = KERNEL_TIMER.start()
    fn = lib().octic_dense_resid_layernorm_fwd_skip if (skip_yb and rs is not None) else lib().octic_dense_resid_layernorm_fwd
    check(fn(_p(x), _p(yb), dt_code(yb.dtype), _p(gamma), _p(rs), int(rps), _p(xout), _p(y), dt_code(out_dtype), _p(w), _p(b),
             _p(stats), rows, d, float(eps), _stream(x)))
    KERNEL_TIMER.stop(t, f"dense_resid_ln_fwd_kernel<{_DTN[out_dtype]}>", rows * d * (8 + yb.element_size() + y.element_size()))
    return xout, y, stats


def dense_layernorm_bwd(gy, x, w, stats, dres, want_param_grads=True):
    """Returns (dx f32 = LN'(gy) + dres, dw, db)."""
    d = x.shape[-1]
    rows = x.numel() // d
    dx = torch.empty_like(x)
    nblk = lib().octic_dense_blocks(rows)
    partials = torch.empty((nblk, 2, d), dtype=torch.float32, device=x.device) if want_param_grads else None
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_layernorm_bwd(_p(gy), dt_code(gy.dtype), _p(x), _p(w), _p(stats), _p(dres), _p(dx),
                                          _p(partials), rows, d, _stream(x)))
    KERNEL_TIMER.stop(t, f"dense_ln_bwd_kernel<{_DTN[gy.dtype]}>",
                      rows * d * (gy.element_size() + 8 + (4 if dres is not None else 0)))
    if not want_param_grads:
        return dx, None, None
    dw = torch.empty(d, dtype=torch.float32, device=x.device)
    db = torch.empty(d, dtype=torch.float32, device=x.device)
    _finish(partials, nblk, d, dw, db, None, _stream(x))
    return dx, dw, db


def dense_ln_bwd_tail_ok(gy, yb, d):
    """Shapes of octic_dense_layernorm_bwd_tail: bf16 cotangent and branch, rows of 256, 512, ... 1280 columns."""
    return gy.dtype == torch.bfloat16 and yb.dtype == torch.bfloat16 and d % 256 == 0 and d <= 1280


def dense_layernorm_bwd_tail(gy, x, w, stats, dres, yb, gamma, rs, rps, want_param_grads=True, want_gamma=True,
                             want_colsum=True, sample_scale=None, rows_per_sample=0, inplace=False):
    """dense_layernorm_bwd followed by scale_residual_bwd on its result, one row pass.
    Returns (dx f32, dw, db, gyb bf16 = rs*gamma*dx, dgamma, gamma * colsum(rs*dx)).
    sample_scale / rows_per_sample: the factor of the branch this norm opens, a promise that the rows of gy are zero where it
    is 0 (octic_dense_layernorm_bwd_tail_skip: those rows of gy, x and stats stay unread, and yb's where rs is 0); a malformed
    mask is a ValueError.
    inplace (needs the mask and a contiguous f32 dres the caller owns): dres is updated in place and returned as dx
    (octic_dense_layernorm_bwd_tail_inplace: the rows of a dropped sample are not written, and not read where rs is 0)."""
    d = x.shape[-1]
    rows = x.numel() // d
    ss, srps = _sample_scale(sample_scale, rows_per_sample, rows, x, "dense_layernorm_bwd_tail")
    if inplace:
        if ss is None or dres is None or dres.dtype != torch.float32 or not dres.is_contiguous() or dres.numel() != x.numel():
            raise ValueError("dense_layernorm_bwd_tail(inplace=True) needs a sample mask and a contiguous float32 dres of x's size")
        dx = dres
    else:
        dx = torch.empty_like(x)
    gyb = torch.empty(x.shape, dtype=yb.dtype, device=x.device)
    nblk = lib().octic_dense_blocks(rows)
    p1 = torch.empty((nblk, 2, d), dtype=torch.float32, device=x.device) if want_param_grads else None
    want2 = want_gamma or want_colsum
    p2 = torch.empty((nblk, 2, d), dtype=torch.float32, device=x.device) if want2 else None
    t = KERNEL_TIMER.start()
    if inplace:
        check(lib().octic_dense_layernorm_bwd_tail_inplace(_p(gy), _p(x), _p(w), _p(stats), _p(dx), _p(p1), _p(yb), _p(gamma),
                                                           _p(rs), int(rps), _p(gyb), _p(p2), rows, d, _p(ss), srps, _stream(x)))
    else:
        check(lib().octic_dense_layernorm_bwd_tail_skip(_p(gy), _p(x), _p(w), _p(stats), _p(dres), _p(dx), _p(p1), _p(yb),
                                                        _p(gamma), _p(rs), int(rps), _p(gyb), _p(p2), rows, d, _p(ss), srps,
                                                        _stream(x)))
    KERNEL_TIMER.stop(t, "dense_ln_bwd_tail_kernel<bf16>", rows * d * (2 + 8 + (4 if dres is not None else 0) + 4))
    dw = db = dgamma = colsum = None
    if want_param_grads:
        dw = torch.empty(d, dtype=torch.float32, device=x.device)
        db = torch.empty(d, dtype=torch.float32, device=x.device)
        _finish(p1, nblk, d, dw, db, None, _stream(x))
    if want2:
        dgamma = torch.empty(d, dtype=torch.float32, device=x.device) if want_gamma else None
        colsum = torch.empty(d, dtype=torch.float32, device=x.device) if want_colsum else None
        _finish(p2, nblk, d, dgamma, colsum, gamma, _stream(x))
    return dx, dw, db, gyb, dgamma, colsum


def _rows2d(t):
    """[..., K] with contiguous rows -> (2-D view, rows, K, row stride)."""
    K = t.shape[-1]
    t2 = t.reshape(-1, K)
    if t2.stride(1) != 1 or (t2.shape[0] > 1 and t2.stride(0) % 8):
        t2 = t2.contiguous()
    return t2, t2.shape[0], K, (t2.stride(0) if t2.shape[0] > 1 else K)


def softmax_center(t, center, inv_temp):
    """softmax((t - center) * inv_temp) over the last dim, f32 (t f32 / bf16 [..., K], center f32 [K] or None)."""
    _require_cuda(t)
    t2, rows, K, ld = _rows2d(t)
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    c = None if center is None else center.reshape(-1).float().contiguous()
    tk = KERNEL_TIMER.start()
    check(lib().octic_softmax_center(_p(t2), dt_code(t2.dtype), ld, _p(c), float(inv_temp), _p(out), rows, K, _stream(t)))
    KERNEL_TIMER.stop(tk, f"softmax_center_kernel<{_DTN[t2.dtype]}>", rows * K * (2 * t2.element_size() + 4))
    return out


def soft_ce_fwd(s, tprob, inv_temp):
    """Per row r of s [N, K]: -sum_k t_k log_softmax(s_r * inv_temp)_k with t = tprob[r % Nt] (tprob f32 [Nt, K] contiguous).
    Returns (loss [N], lse [N], tsum [N]) f32."""
    _require_cuda(s)
    s2, rows, K, ld = _rows2d(s)
    if tprob.dtype != torch.float32 or not tprob.is_contiguous() or tprob.shape[-1] != K:
        raise ValueError("soft_ce_fwd: tprob must be a contiguous f32 [Nt, K] tensor")
    nt = tprob.numel() // K
    loss, lse, tsum = (torch.empty(rows, dtype=torch.float32, device=s.device) for _ in range(3))
    tk = KERNEL_TIMER.start()
    check(lib().octic_soft_ce_fwd(_p(s2), dt_code(s2.dtype), ld, _p(tprob), nt, float(inv_temp), _p(loss), _p(lse), _p(tsum),
                                  rows, K, _stream(s)))
    KERNEL_TIMER.stop(tk, f"soft_ce_fwd_kernel<{_DTN[s2.dtype]}>", rows * K * (s2.element_size() + 4))
    return loss, lse, tsum


def soft_ce_bwd(s, tprob, inv_temp, g, lse, tsum):
    """d loss / d s for soft_ce_fwd, in s's dtype ([N, K] contiguous)."""
    s2, rows, K, ld = _rows2d(s)
    nt = tprob.numel() // K
    ds = torch.empty((rows, K), dtype=s2.dtype, device=s.device)
    g = g.reshape(-1).float().contiguous()
    tk = KERNEL_TIMER.start()
    check(lib().octic_soft_ce_bwd(_p(s2), dt_code(s2.dtype), ld, _p(tprob), nt, float(inv_temp), _p(g), _p(lse), _p(tsum),
                                  _p(ds), K, rows, K, _stream(s)))
    KERNEL_TIMER.stop(tk, f"soft_ce_bwd_kernel<{_DTN[s2.dtype]}>", rows * K * (2 * s2.element_size() + 4))
    return ds.view(s.shape)


def _sinkhorn_rows2d(x):
    """The logits of a Sinkhorn pass: a 2-D f32 / bf16 tensor as (view with 16-byte aligned rows, rows, K, row stride)."""
    _require_cuda(x)
    if x.dim() != 2:
        raise ValueError("sinkhorn passes take 2-D logits [rows, K]")
    if x.data_ptr() % 16:
        x = x.clone(memory_format=torch.contiguous_format)
    return _rows2d(x)


def sinkhorn_rows(x, inv_temp, u=None):
    """Sample-sum pass of csrc/ssl_loss.hip: (rowmax [rows], c [rows]) f32, rowmax[b] = max_k x[b, k] and
    c[b] = sum_k u[k] exp((x[b, k] - rowmax[b]) * inv_temp) (u f32 [K] contiguous, or None: 1)."""
    x2, rows, K, ld = _sinkhorn_rows2d(x)
    rowmax, c = (torch.empty(rows, dtype=torch.float32, device=x.device) for _ in range(2))
    tk = KERNEL_TIMER.start()
    check(lib().octic_sinkhorn_rows(_p(x2), dt_code(x2.dtype), ld, float(inv_temp), _p(u), _p(rowmax), _p(c), rows, K,
                                    _stream(x)))
    KERNEL_TIMER.stop(tk, f"sinkhorn_rows_kernel<{_DTN[x2.dtype]}>", rows * K * x2.element_size())
    return rowmax, c


def sinkhorn_protos(x, inv_temp, shift, weight):
    """Prototype-sum pass: r [K] f32, r[k] = sum_b weight[b] exp((x[b, k] - shift[b]) * inv_temp) (shift, weight f32 [rows]);
    per-slab partial sums in a fixed order, no atomics."""
    x2, rows, K, ld = _sinkhorn_rows2d(x)
    slabs = lib().octic_sinkhorn_slabs(rows)
    if slabs < 0:
        check(slabs)
    r = torch.empty(K, dtype=torch.float32, device=x.device)
    part = torch.empty((slabs, K), dtype=torch.float32, device=x.device) if slabs > 1 else None
    tk = KERNEL_TIMER.start()
    check(lib().octic_sinkhorn_protos(_p(x2), dt_code(x2.dtype), ld, float(inv_temp), _p(shift), _p(weight), _p(part), _p(r),
                                      rows, K, _stream(x)))
    KERNEL_TIMER.stop(tk, f"sinkhorn_protos_kernel<{_DTN[x2.dtype]}>", rows * K * x2.element_size() + (slabs > 1) * slabs * K * 8)
    return r


def sinkhorn_final(x, inv_temp, u):
    """Final pass: out [rows, K] contiguous f32, out[b, :] = u E[b, :] / sum_k u[k] E[b, k], E[b, k] = exp((x[b, k] - rowmax[b]) * inv_temp)."""
    x2, rows, K, ld = _sinkhorn_rows2d(x)
    out = torch.empty((rows, K), dtype=torch.float32, device=x.device)
    tk = KERNEL_TIMER.start()
    check(lib().octic_sinkhorn_final(_p(x2), dt_code(x2.dtype), ld, float(inv_temp), _p(u), _p(out), rows, K, _stream(x)))
    KERNEL_TIMER.stop(tk, f"sinkhorn_final_kernel<{_DTN[x2.dtype]}>", rows * K * (2 * x2.element_size() + 4))
    return out


def koleo_ok(groups, n, D):
    """The KoLeo kernels of csrc/koleo.hip take `groups` groups of n rows of D elements (octic_koleo_ok: the only place the range
    lives)."""
    return bool(lib().octic_koleo_ok(int(groups), int(n), int(D)))


def _koleo_rows2d(x, groups):
    """x [groups * n, D] f32 / bf16 as (view with unit column stride and 16-byte aligned rows, n, D, row stride)."""
    _require_cuda(x)
    if x.dim() != 2 or groups < 1 or x.shape[0] % groups:
        raise ValueError("koleo: x must be [groups * n, D]")
    if x.stride(1) != 1 or x.data_ptr() % 16 or (x.stride(0) * x.element_size()) % 16:
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
    return x, x.shape[0] // groups, x.shape[1], x.stride(0)


def koleo_fwd(x, groups, eps=1e-8):
    """KoLeo terms of `groups` independent groups of consecutive rows of x [groups * n, D] (f32 / bf16) in one launch:
    (term [rows] f32 = -log(dist + eps), nn [rows] int32 = group-local index of the nearest other row of the group by the dot of
    the normalised rows, lowest index on ties, inv [rows] f32 = 1 / max(||x_i||, eps), dist [rows] f32 = ||xh_i - xh_nn + 1e-8||)."""
    x2, n, D, ld = _koleo_rows2d(x, groups)
    rows = groups * n
    term, inv, dist = (torch.empty(rows, dtype=torch.float32, device=x.device) for _ in range(3))
    nn = torch.empty(rows, dtype=torch.int32, device=x.device)
    tk = KERNEL_TIMER.start()
    check(lib().octic_koleo_fwd(_p(x2), dt_code(x2.dtype), ld, groups, n, D, float(eps), _p(term), _p(nn), _p(inv), _p(dist),
                                _stream(x)))
    KERNEL_TIMER.stop(tk, f"koleo_fwd_kernel<{_DTN[x2.dtype]}>", rows * (n + 1) * D * x2.element_size())
    return term, nn, inv, dist


def koleo_bwd(x, groups, gterm, nn, inv, dist, eps=1e-8):
    """d loss / d x for koleo_fwd from gterm = d loss / d term [rows], in x's dtype ([groups * n, D] contiguous); the rows that
    chose row i are gathered in ascending order by its workgroup (no atomics)."""
    x2, n, D, ld = _koleo_rows2d(x, groups)
    rows = groups * n
    dx = torch.empty((rows, D), dtype=x2.dtype, device=x.device)
    gterm = gterm.reshape(-1).float().contiguous()
    tk = KERNEL_TIMER.start()
    check(lib().octic_koleo_bwd(_p(x2), dt_code(x2.dtype), ld, groups, n, D, float(eps), _p(gterm), _p(nn), _p(inv), _p(dist),
                                _p(dx), D, _stream(x)))
    KERNEL_TIMER.stop(tk, f"koleo_bwd_kernel<{_DTN[x2.dtype]}>", rows * 4 * D * x2.element_size())
    return dx


# ------------------------------------------------------------------ input rows of the DINO / iBOT heads (csrc/dino_head.hip)
def _aligned_rows2d(x, what):
    """x [rows, D] f32 / bf16 as a view with unit column stride and 16-byte aligned rows (a copy where it has neither)."""
    _require_cuda(x)
    if x.dim() != 2:
        raise ValueError(f"{what}: expected [rows, D], got {tuple(x.shape)}")
    dt_code(x.dtype)
    if x.stride(1) != 1 or x.data_ptr() % 16 or (x.shape[0] > 1 and (x.stride(0) * x.element_size()) % 16):
        x = x.contiguous()
        if x.data_ptr() % 16:
            x = x.clone(memory_format=torch.contiguous_format)
    return x


def _ldrow(x):
    """Row stride of a 2-D view (a one-row tensor's stride is whatever torch left there)."""
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


HEAD_ROWS_MAX_SEGMENTS = 4
_HEAD_TABLES = {}


def _head_segment(src, idx, out_row0, D, dtype):
    """One octic_head_segment (8 int64 words) for the rows of src - [n, D], or [B, P, D] read as its B * P rows - taken through
    idx (int64 on the device) or in order."""
    if src.dtype != dtype or src.shape[-1] != D or src.dim() not in (2, 3) or src.stride(-1) != 1:
        raise ValueError(f"head_rows: sources must be {dtype} [n, {D}] or [B, P, {D}] with unit column stride, got "
                         f"{tuple(src.shape)} {src.dtype}")
    es = src.element_size()
    if src.dim() == 2:
        src_rows, inner, outer_ld, inner_ld = src.shape[0], 1, src.stride(0), 0
        lds = (outer_ld,) if src_rows > 1 else ()
    else:
        src_rows, inner, outer_ld, inner_ld = src.shape[0] * src.shape[1], src.shape[1], src.stride(0), src.stride(1)
        lds = ((outer_ld,) if src.shape[0] > 1 else ()) + ((inner_ld,) if src.shape[1] > 1 else ())
    if src.data_ptr() % 16 or any((ld * es) % 16 for ld in lds):
        raise ValueError("head_rows: source rows must be 16-byte aligned")
    if idx is not None and (not idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous()):
        raise ValueError("head_rows: idx must be a contiguous int64 vector on the device")
    n = src_rows if idx is None else idx.numel()
    return (src.data_ptr(), 0 if idx is None else idx.data_ptr(), n, max(inner, 1), outer_ld, inner_ld, int(out_row0), src_rows)


def head_rows(segments, out, scatter=False):
    """The head's input rows (octic_head_rows).  segments: up to four (src, idx or None, out_row0) - see _head_segment; the rows
    of a segment own out[out_row0 : out_row0 + n].  scatter False: out [rows_out, D] receives the source rows, every row no
    segment covers is +0.  scatter True: the rows of out are written back to their sources (distinct indices: plain stores); the
    sources are edited in place."""
    import numpy as np
    _require_cuda(out)
    if out.dim() != 2 or out.stride(1) != 1 or not 1 <= len(segments) <= HEAD_ROWS_MAX_SEGMENTS:
        raise ValueError("head_rows: out must be [rows_out, D] with unit column stride, with 1 .. 4 segments")
    rows_out, D = out.shape
    words = [_head_segment(src, idx, r0, D, out.dtype) for src, idx, r0 in segments]
    spans = sorted((w[6], w[6] + w[2]) for w in words if w[2])
    if any(a < 0 or b > rows_out for a, b in spans) or any(spans[i][1] > spans[i + 1][0] for i in range(len(spans) - 1)):
        raise ValueError("head_rows: segments must lie inside out and not overlap")
    key = (out.device, tuple(words))
    table = _HEAD_TABLES.get(key)
    if table is None:                              # (activations keep their addresses from step to step: one upload per layout)
        if len(_HEAD_TABLES) >= 256:
            _HEAD_TABLES.clear()
        host = torch.from_numpy(np.asarray(words, dtype=np.int64).reshape(-1)).pin_memory()
        table = _HEAD_TABLES[key] = host.to(out.device, non_blocking=True)
    tk = KERNEL_TIMER.start()
    check(lib().octic_head_rows(_p(table), len(words), rows_out, D, dt_code(out.dtype), _p(out), _ldrow(out), int(bool(scatter)),
                                _stream(out)))
    moved = rows_out if not scatter else sum(w[2] for w in words)
    KERNEL_TIMER.stop(tk, f"head_rows_kernel<{'scatter' if scatter else 'gather'},{_DTN[out.dtype]}>",
                      2 * moved * D * out.element_size())
    return out


# ------------------------------------------------------------ the normalisations of the DINO / iBOT heads (csrc/dino_norm.hip)
def l2norm_ok(rows, D):
    """Shapes the L2-normalisation row kernels take (octic_l2norm_ok: the only place the range lives)."""
    return bool(lib().octic_l2norm_ok(int(rows), int(D)))


def _l2_rows(t, what, dtype=None):
    """t as [rows, D] f32 / bf16 with unit column stride and 16-byte aligned rows, or a ValueError."""
    _require_cuda(t)
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"{what}: expected [rows, D] with unit column stride, got {tuple(t.shape)} strides {t.stride()}")
    dt_code(t.dtype)
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{what}: expected {dtype}, got {t.dtype}")
    if t.data_ptr() % 16 or (t.shape[0] > 1 and (t.stride(0) * t.element_size()) % 16):
        raise ValueError(f"{what}: rows must be 16-byte aligned")
    return t


def l2norm_rows(x, eps=1e-12, out_dtype=None):
    """F.normalize(x, dim=-1, p=2, eps) of x [rows, D] (f32 / bf16) -> (y [rows, D] in out_dtype (default: x's), inv [rows] f32 =
    1 / max(||x||, eps)) - octic_l2norm_rows_fwd: f32 sum of squares, one rounding."""
    x = _l2_rows(x, "l2norm_rows")
    rows, D = x.shape
    out_dtype = out_dtype or x.dtype
    dt_code(out_dtype)
    if not l2norm_ok(rows, D):
        raise ValueError(f"l2norm_rows: [rows, D] = {tuple(x.shape)} is outside the kernel's range (octic_l2norm_ok)")
    y = torch.empty((rows, D), dtype=out_dtype, device=x.device)
    inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_l2norm_rows_fwd(_p(x), dt_code(x.dtype), _ldrow(x), rows, D, float(eps), _p(y), dt_code(out_dtype), D, _p(inv),
                                      _stream(x)))
    KERNEL_TIMER.stop(t, f"l2norm_fwd_kernel<{_DTN[x.dtype]},{_DTN[out_dtype]}>", rows * D * (x.element_size() + y.element_size()))
    return y, inv


def l2norm_rows_bwd(g, x, inv, eps=1e-12):
    """dx (x's dtype) of l2norm_rows from the cotangent g [rows, D] (f32 / bf16) of y, x and the saved inv
    (octic_l2norm_rows_bwd): inv (g - yh (yh . g)) with yh = x inv, and g inv on the rows whose norm is below eps."""
    x = _l2_rows(x, "l2norm_rows_bwd: x")
    g = _l2_rows(g, "l2norm_rows_bwd: g")
    rows, D = x.shape
    if tuple(g.shape) != (rows, D) or not l2norm_ok(rows, D):
        raise ValueError(f"l2norm_rows_bwd: g {tuple(g.shape)} must match x {tuple(x.shape)} inside the kernel's range")
    if not inv.is_cuda or inv.dtype != torch.float32 or tuple(inv.shape) != (rows,) or not inv.is_contiguous():
        raise ValueError("l2norm_rows_bwd: inv must be the contiguous f32 [rows] vector of l2norm_rows")
    dx = torch.empty((rows, D), dtype=x.dtype, device=x.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_l2norm_rows_bwd(_p(g), dt_code(g.dtype), _ldrow(g), _p(x), dt_code(x.dtype), _ldrow(x), _p(inv), rows, D,
                                      float(eps), _p(dx), D, _stream(x)))
    KERNEL_TIMER.stop(t, f"l2norm_bwd_kernel<{_DTN[g.dtype]},{_DTN[x.dtype]}>", rows * D * (g.element_size() + 2 * x.element_size()))
    return dx


WEIGHT_NORM_MAX_K = 2048       # csrc/dino_norm.hip: a row of v lives in one wave's registers


def weight_norm_ok(N, K):
    """Shapes octic_weight_norm_prep (with the transposed operand) and octic_weight_norm_bwd take."""
    return N >= 8 and N % 8 == 0 and N < 2 ** 29 and 8 <= K <= WEIGHT_NORM_MAX_K and K % 8 == 0


def _wn_operands(v, g, what):
    _require_cuda(v)
    if v.dim() != 2 or v.dtype != torch.float32 or not v.is_contiguous() or v.data_ptr() % 16:
        raise ValueError(f"{what}: weight_v must be a contiguous, 16-byte aligned f32 [N, K] tensor on the device")
    N, K = v.shape
    if not g.is_cuda or g.dtype != torch.float32 or g.numel() != N or not g.is_contiguous():
        raise ValueError(f"{what}: weight_g must be a contiguous f32 [N, 1] tensor on the device")
    if N < 1 or N >= 2 ** 29 or K < 8 or K > WEIGHT_NORM_MAX_K or K % 8:
        raise ValueError(f"{what}: [N, K] = {(N, K)} is outside the kernel's range (K % 8 == 0, 8 <= K <= {WEIGHT_NORM_MAX_K})")
    return N, K


def weight_norm_prep(v, g, want_wt=True, wt_out=None):
    """The bf16 operands of a weight-normed linear layer (nn.utils.weight_norm, dim 0) from weight_v [N, K] and weight_g [N, 1],
    f32, in one pass: (W [N, K] = bf16(g v / ||v||_row), W^T [K, N] or None, norms [N] f32) - octic_weight_norm_prep.  The f32
    weight is never written.  want_wt False: the transposed operand (the input-gradient GEMM's) is not produced and wt_out, if
    given, is left alone."""
    N, K = _wn_operands(v, g, "weight_norm_prep")
    w = torch.empty((N, K), dtype=torch.bfloat16, device=v.device)
    wt = None
    if want_wt:
        if N % 8:
            raise ValueError("weight_norm_prep: the transposed operand needs N % 8 == 0")
        wt = wt_out if wt_out is not None else torch.empty((K, N), dtype=torch.bfloat16, device=v.device)
        if (not wt.is_cuda or wt.dtype != torch.bfloat16 or tuple(wt.shape) != (K, N) or not wt.is_contiguous()
                or wt.data_ptr() % 16):
            raise ValueError("weight_norm_prep: wt_out must be a contiguous, 16-byte aligned bf16 [K, N] tensor on the device")
    norms = torch.empty(N, dtype=torch.float32, device=v.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_weight_norm_prep(_p(v), _p(g), N, K, _p(w), _p(wt), _p(norms), _stream(v)))
    KERNEL_TIMER.stop(t, f"weight_norm_prep_kernel<{'nt' if want_wt else 'n'}>", N * K * (4 + (4 if want_wt else 2)) + 8 * N)
    return w, wt, norms


def weight_norm_bwd(dw, v, g, norms):
    """(dv [N, K], dg [N, 1]) of the weight-normed weight from its f32 gradient dw [N, K], weight_v, weight_g and the norms
    weight_norm_prep saved (octic_weight_norm_bwd; autograd of torch._weight_norm, f32)."""
    N, K = _wn_operands(v, g, "weight_norm_bwd")
    if (not dw.is_cuda or dw.dtype != torch.float32 or tuple(dw.shape) != (N, K) or not dw.is_contiguous()
            or dw.data_ptr() % 16):
        raise ValueError("weight_norm_bwd: dw must be a contiguous, 16-byte aligned f32 [N, K] tensor on the device")
    if not norms.is_cuda or norms.dtype != torch.float32 or tuple(norms.shape) != (N,) or not norms.is_contiguous():
        raise ValueError("weight_norm_bwd: norms must be the contiguous f32 [N] vector of weight_norm_prep")
    dv = torch.empty((N, K), dtype=torch.float32, device=v.device)
    dg = torch.empty(g.shape, dtype=torch.float32, device=v.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_weight_norm_bwd(_p(dw), _p(v), _p(g), _p(norms), N, K, _p(dv), _p(dg), _stream(v)))
    KERNEL_TIMER.stop(t, "weight_norm_bwd_kernel", 12 * N * K + 12 * N)
    return dv, dg


def scale_residual_fwd(x, y, gamma, rs, rps):
    """out = x + rs[row // rps] * gamma * y   (x f32, y f32/bf16, same shape [..., d])."""
    _require_cuda(x)
    d = x.shape[-1]
    rows = x.numel() // d
    out = torch.empty_like(x)
    t = KERNEL_TIMER.start()
    check(lib().octic_scale_residual_fwd(_p(x), _p(y), dt_code(y.dtype), _p(gamma), _p(rs), int(rps), _p(out), rows, d,
                                         _stream(x)))
    KERNEL_TIMER.stop(t, f"scale_residual_fwd_kernel<{_DTN[y.dtype]}>", rows * d * (8 + y.element_size()))
    return out


def scale_residual_fwd_rows_(stream, rowmap, x, y, gamma, rs, rps):
    """In place on the f32 stream: stream[rowmap[r]] = x[r] + rs[r // rps] * gamma * y[r]  (x, y compact)."""
    _require_cuda(x)
    d = x.shape[-1]
    rows = rowmap.numel()
    _check_rowmap(rowmap, rows)
    t = KERNEL_TIMER.start()
    check(lib().octic_scale_residual_fwd_rows(_p(x), _p(y), dt_code(y.dtype), _p(gamma), _p(rs), int(rps), _p(stream), rows, d,
                                              _p(rowmap), _stream(x)))
    KERNEL_TIMER.stop(t, f"scale_residual_fwd_kernel<{_DTN[y.dtype]},rows>", rows * d * (8 + y.element_size()))
    return stream


def scale_residual_bwd(gout, y, gamma, rs, rps, want_gamma=True, want_colsum=True, rowmap=None):
    """Returns (gy in y's dtype, dgamma, gamma * colsum(rs*gout) = bias gradient of the producer of y).  rowmap: the compact
    rows of y are rows rowmap[r] of gout (the cotangent of a stream of which the branch saw a subset)."""
    d = gout.shape[-1]
    rows = gout.numel() // d if rowmap is None else rowmap.numel()
    if rowmap is not None:
        _check_rowmap(rowmap, rows)
    gy = torch.empty(gout.shape if rowmap is None else y.shape, dtype=y.dtype, device=gout.device)
    nblk = lib().octic_dense_blocks(rows)
    want = want_gamma or want_colsum
    partials = torch.empty((nblk, 2, d), dtype=torch.float32, device=gout.device) if want else None
    t = KERNEL_TIMER.start()
    check(lib().octic_scale_residual_bwd_rows(_p(gout), _p(y), dt_code(y.dtype), _p(gamma), _p(rs), int(rps), _p(gy),
                                              _p(partials), rows, d, _p(rowmap), _stream(gout)))
    KERNEL_TIMER.stop(t, f"scale_residual_bwd_kernel<{_DTN[y.dtype]}>", rows * d * (4 + 2 * y.element_size()))
    if not want:
        return gy, None, None
    dgamma = torch.empty(d, dtype=torch.float32, device=gout.device) if want_gamma else None
    colsum = torch.empty(d, dtype=torch.float32, device=gout.device) if want_colsum else None
    _finish(partials, nblk, d, dgamma, colsum, gamma, _stream(gout))
    return gy, dgamma, colsum


def dense_gelu_bwd(h, g, want_colsum=True):
    """dh = gelu'(h) * g for bf16 [..., d]; also the column sums of dh (f32 [d]) when asked."""
    _require_cuda(h)
    d = h.shape[-1]
    rows = h.numel() // d
    dh = torch.empty_like(h)
    nblk = lib().octic_dense_gelu_blocks()
    partials = torch.empty((nblk, d), dtype=torch.float32, device=h.device) if want_colsum else None
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_gelu_bwd(_p(h), _p(g), _p(dh), _p(partials), rows, d, _stream(h)))
    KERNEL_TIMER.stop(t, "dense_gelu_bwd_kernel", rows * d * 6)
    if not want_colsum:
        return dh, None
    out = torch.empty(d, dtype=torch.float32, device=h.device)
    half = d // 2
    _finish(partials, nblk, half, out, None, None, _stream(h), out1_ptr=out.data_ptr() + 4 * half)
    return dh, out


def _swiglu_rows(t, width, what):
    """t as [rows, width] with unit column stride: a 2-D tensor as it is (its row stride travels to the kernel), anything else
    contiguous and flattened."""
    if t.dim() != 2:
        t = t.reshape(-1, t.shape[-1]) if t.is_contiguous() else t.contiguous().view(-1, t.shape[-1])
    if t.dtype != torch.bfloat16 or t.shape[1] != width or t.stride(1) != 1:
        raise ValueError(f"swiglu: {what} must be bf16 [rows, {width}] with contiguous columns, got {tuple(t.shape)} {t.dtype}")
    return t


def swiglu_fwd(x12, H, out=None):
    """a = silu(x1) * x2 for x12 = [x1 | x2] bf16 [..., 2H] (the gate of DINOv2's SwiGLU FFN) -> bf16 [..., H].
    out: a 2-D [rows, H] destination (any row stride the library takes)."""
    _require_cuda(x12)
    lead = x12.shape[:-1]
    x2d = _swiglu_rows(x12, 2 * H, "x12")
    rows = x2d.shape[0]
    a = torch.empty((rows, H), dtype=torch.bfloat16, device=x12.device) if out is None else _swiglu_rows(out, H, "out")
    t = KERNEL_TIMER.start()
    check(lib().octic_swiglu_fwd(_p(x2d), x2d.stride(0), _p(a), a.stride(0), rows, H, _stream(x12)))
    KERNEL_TIMER.stop(t, "swiglu_fwd_kernel", rows * H * 6)
    return a.view(*lead, H) if out is None else out


def swiglu_bwd(x12, ga, want_colsum=True, out=None):
    """(dx12, db12): the cotangent of x12 = [x1 | x2] from ga, the cotangent of silu(x1) * x2, and - when asked - its f32
    column sums [2H] (the bias gradient of w12, in w12.bias order).  out: a 2-D [rows, 2H] destination."""
    _require_cuda(x12)
    H = ga.shape[-1]
    x2d, g2d = _swiglu_rows(x12, 2 * H, "x12"), _swiglu_rows(ga, H, "ga")
    rows = x2d.shape[0]
    if g2d.shape[0] != rows:
        raise ValueError("swiglu_bwd: x12 and ga differ in rows")
    d = torch.empty((rows, 2 * H), dtype=torch.bfloat16, device=x12.device) if out is None else _swiglu_rows(out, 2 * H, "out")
    nblk = lib().octic_swiglu_blocks()
    partials = torch.empty((nblk, 2 * H), dtype=torch.float32, device=x12.device) if want_colsum and rows else None
    t = KERNEL_TIMER.start()
    check(lib().octic_swiglu_bwd(_p(x2d), x2d.stride(0), _p(g2d), g2d.stride(0), _p(d), d.stride(0), _p(partials), rows, H,
                                 _stream(x12)))
    KERNEL_TIMER.stop(t, "swiglu_bwd_kernel", rows * H * 10)
    dx = d.view(x12.shape) if out is None else out
    if not want_colsum:
        return dx, None
    if partials is None:
        return dx, torch.zeros(2 * H, dtype=torch.float32, device=x12.device)
    db = torch.empty(2 * H, dtype=torch.float32, device=x12.device)
    _finish(partials, nblk, H, db, None, None, _stream(x12), out1_ptr=db.data_ptr() + 4 * H)
    return dx, db


# ------------------------------------------------------------------------------------------ dense MFMA GEMMs
_DG_WS = {}
# octic_dense_gemm_workspace_bytes depends on the override table (OCTIC_ROUTE_DENSE_SPLIT makes a problem split that otherwise
# would not): a workspace sized under one table never serves a launch planned under another
_lib.on_route_override(_DG_WS.clear)


def _dense_ws(M, N, K, dev):
    """Split-K workspace of one (M,N,K) problem, cached per stream-ordered use (launches on one stream are serial) until
    the next _lib.route_override."""
    key = (M, N, K, dev)
    ws = _DG_WS.get(key)
    if ws is None:
        ws = _DG_WS[key] = torch.zeros(int(lib().octic_dense_gemm_workspace_bytes(M, N, K)), dtype=torch.uint8, device=dev)
    return ws


def dense_colsum(g, sample_scale=None, rows_per_sample=0):
    """f32 column sums of a bf16 [rows, d] tensor (unit column stride): the bias gradient of a dense nn.Linear.
    sample_scale / rows_per_sample: a promise that the rows of a sample are zero where its entry is 0 (they stay unread); a
    malformed mask is a ValueError."""
    _require_cuda(g)
    rows, d = g.shape
    if g.stride(1) != 1:
        raise ValueError("dense_colsum: rows must be contiguous along d")
    ss, srps = _sample_scale(sample_scale, rows_per_sample, rows, g, "dense_colsum")
    nblk = lib().octic_dense_gelu_blocks()
    partials = torch.empty((nblk, d), dtype=torch.float32, device=g.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_colsum_skip(_p(g), rows, d, g.stride(0), _p(partials), _p(ss), srps, _stream(g)))
    KERNEL_TIMER.stop(t, "dense_colsum_kernel", rows * d * 2)
    out = torch.empty(d, dtype=torch.float32, device=g.device)
    half = d // 2
    _finish(partials, nblk, half, out, None, None, _stream(g), out1_ptr=out.data_ptr() + 4 * half)
    return out


def dense_plan(M, N, K, mode, tokens):
    """(tile width, colsum slab rows, per-image panels?, main-launch workgroups) of octic_dense_gemm_nt_tokens."""
    out = _lib.plan("octic_dense_gemm_plan", M, N, K, mode, int(tokens))
    if out is None:
        check(-1)
    return out[0], out[1], bool(out[2]), out[3]


def dense_plan_dropped(M, N, K, mode, tokens, rows_per_sample):
    """dense_plan for a launch under a stochastic-depth mask (octic_dense_gemm_plan_dropped)."""
    out = _lib.plan("octic_dense_gemm_plan_dropped", M, N, K, mode, int(tokens), int(rows_per_sample))
    if out is None:
        check(-1)
    return out[0], out[1], bool(out[2]), out[3]


def dense_plan_adaptive(M, N, K, mode, tokens, rows_per_sample):
    """(adaptive kernel takes it?, main-launch workgroups, wide width, narrow width, most live panels that run narrow) of a masked
    octic_dense_gemm_nt_tokens_adaptive launch."""
    out = (ctypes.c_int * 5)()
    check(lib().octic_dense_gemm_plan_adaptive(M, N, K, mode, int(tokens), int(rows_per_sample), out))
    return bool(out[0]), out[1], out[2], out[3], out[4]


def _dense_narrow():
    from . import functional          # (functional imports this module)
    return functional.DENSE_NARROW_DROPPED


def dense_plan_adaptive_cls(M, N, K, mode, tokens, rows_per_sample):
    """(folded kernel takes it?, workgroups of the launch, class-token workgroups at its end, class-token items of the busiest
    one, tile workgroups in front) of a masked octic_dense_gemm_nt_tokens_adaptive_cls launch with fold_cls on."""
    out = (ctypes.c_int * 5)()
    check(lib().octic_dense_gemm_plan_adaptive_cls(M, N, K, mode, int(tokens), int(rows_per_sample), out))
    return bool(out[0]), out[1], out[2], out[3], out[4]


def _dense_cls_fold():
    from . import functional          # (functional imports this module)
    return functional.DENSE_NARROW_DROPPED and functional.DENSE_CLS_FOLD


_DG_IMAGE_PLANS = {}
_lib.on_route_override(_DG_IMAGE_PLANS.clear)


def dense_plan_image(M, N, K, mode, tokens, rows_per_sample, drop, masked=True):
    """(leaves the former call's plan for per-image panels?, workgroups of the main launch, class-token workgroups at its end,
    class-token items of the busiest one, tile workgroups in front, tile width, colsum slab rows, per-image panels in force?) of
    an octic_dense_gemm_nt_tokens_image launch under the mask of a branch with drop probability `drop`."""
    key = (M, N, K, mode, int(tokens), int(rows_per_sample), bool(masked), float(drop or 0.0))
    ans = _DG_IMAGE_PLANS.get(key)
    if ans is None:
        out = (ctypes.c_int * 8)()
        check(lib().octic_dense_gemm_plan_image(M, N, K, mode, key[4], key[5], int(key[6]), key[7], out))
        ans = _DG_IMAGE_PLANS[key] = (bool(out[0]), out[1], out[2], out[3], out[4], out[5], out[6], bool(out[7]))
    return ans


def _dense_image():
    from . import functional          # (functional imports this module)
    return functional.DENSE_NT_SKIP_DROPPED and functional.DENSE_IMAGE_DROPPED


def _dense_entry(M, N, K, mode, tokens, ss, srps, fold_cls, drop):
    """(C entry point, its arguments between `tokens` and the stream, tile width, colsum slab rows) of a dense_gemm_nt call: the
    switches of functional pick the entry (the library decides which launches it changes); width and slab rows are the plan's in
    force, with a mask or without - colsum rows and the timer name belong to it."""
    if ss is not None and drop is not None and float(drop) > 0.0 and _dense_image():
        image = dense_plan_image(M, N, K, mode, tokens, srps, drop)
        if image[0]:                                          # (not taken: the former call, the former plan)
            return lib().octic_dense_gemm_nt_tokens_image, (0, float(drop)), image[5], image[6]
    width, slab_rows = dense_plan(M, N, K, mode, tokens)[:2]
    if ss is not None and fold_cls and _dense_cls_fold():
        return lib().octic_dense_gemm_nt_tokens_adaptive_cls, (1,), width, slab_rows
    # a masked launch may choose its tile width on the device (functional.DENSE_NARROW_DROPPED)
    if ss is not None and _dense_narrow():
        return lib().octic_dense_gemm_nt_tokens_adaptive, (), width, slab_rows
    return lib().octic_dense_gemm_nt_tokens_skip, (), width, slab_rows


def dense_gemm_nt(a, b, mode=0, bias=None, gamma=None, rs=None, rps=1, x=None, h=None, name=None, want_colsum=False,
                  tokens=0, sample_scale=None, rows_per_sample=0, fold_cls=False, drop=None):
    """C[M,N] = a[M,K] @ b[N,K]^T on the hand-written MFMA kernel (csrc/dense_gemm.hip) with a fused tail:
    mode 0 -> c ; 1 -> (c, gelu(c)) ; 2 -> (c, x + rs*gamma*c) ; 3 -> gelu'(h) * c (want_colsum: also the f32 column
    sums of that result) ; 4 -> (gelu'(c), gelu(c)) ; 5 -> h * c with h = the factor of mode 4 (want_colsum as 3) ;
    6 -> gelu(c) only.
    a, b bf16 2-D, K contiguous.  tokens: the rows are whole images of that many tokens ([B, tokens, K] flattened) - 257 lets the
    launch use per-image row panels + the class-token kernel (octic_dense_gemm_nt_tokens); 0 = unknown.
    sample_scale / rows_per_sample: the stochastic-depth mask of octic_dense_gemm_nt_tokens_skip - f32 [M / rows_per_sample] on
    the device, 0 = every reader of that sample's output rows accepts the computed result or +0 (never with mode 2); a
    malformed mask is a ValueError.
    fold_cls: the caller expects the mask to drop enough samples for the class-token rows to ride in the main launch
    (functional.dense_cls_fold; octic_dense_gemm_nt_tokens_adaptive_cls decides which launches can) - same bits either way.
    drop: the probability the mask was drawn with, where the caller knows it: a masked launch may then leave classic row panels
    for per-image ones (functional.DENSE_IMAGE_DROPPED; octic_dense_gemm_nt_tokens_image decides which launches do)."""
    _require_cuda(a)
    M, K = a.shape
    N = b.shape[0]
    if a.stride(1) != 1 or b.stride(1) != 1 or b.shape[1] != K:
        raise ValueError("dense_gemm_nt: operands must be [M,K] / [N,K] with contiguous K")
    c = torch.empty((M, N), dtype=torch.bfloat16, device=a.device)
    c2 = torch.empty_like(c) if mode in (1, 4) else None
    out = torch.empty((M, N), dtype=torch.float32, device=a.device) if mode == 2 else None
    ws = _dense_ws(M, N, K, a.device)
    tokens = int(tokens) if (tokens and M % int(tokens) == 0) else 0
    if sample_scale is not None and mode == 2:
        raise ValueError("dense_gemm_nt: the fused residual tail (mode 2) takes no sample_scale")
    ss, srps = _sample_scale(sample_scale, rows_per_sample, M, a, "dense_gemm_nt")
    entry, extra, width, slab_rows = _dense_entry(M, N, K, mode, tokens, ss, srps, fold_cls, drop)
    cs_rows = slab_rows if (mode in (3, 5) and want_colsum) else 0
    cs = torch.empty((cs_rows, N), dtype=torch.float32, device=a.device) if cs_rows else None
    t = KERNEL_TIMER.start()
    check(entry(_p(a), _p(b), M, N, K, a.stride(0), b.stride(0), mode, _p(c), _p(c2), N, _p(bias), _p(gamma), _p(rs), int(rps),
                _p(x), _p(out), _p(h), _p(cs), _p(ss), srps, _p(ws), tokens, *extra, _stream(a)))
    if t is not None:
        nb = 2 * (M * K + N * K + M * N * (2 if mode in (1, 3, 4, 5) else 1)) + (8 * M * N if mode == 2 else 0)
        # "@320": the launch ran the 256 x 320 tile (kernel symbol dense_nt_kernel<0, 5>), else <mode, 4>
        # (with per-image panels the timed interval also holds the class-token launch behind the panels')
        wide = "@320" if width == 320 else ""
        KERNEL_TIMER.stop(t, (name or f"dense_nt_kernel<{mode}>") + wide, nb, 2.0 * M * N * K)
    if mode in (1, 4):
        return c, c2
    if mode == 2:
        return c, out
    if cs is not None:
        colsum = torch.empty(N, dtype=torch.float32, device=a.device)
        _finish(cs, cs_rows, N // 2, colsum, None, None, _stream(a), out1_ptr=colsum.data_ptr() + 2 * N)
        return c, colsum
    return c


# ------------------------------------------------------------------------------------------ float32 dense GEMMs (csrc/dense_f32.hip)
@torch.compiler.assume_constant_result
def _dense_f32_query(op, M, N, K, ld_max):
    return _lib.plan("octic_dense_f32_plan", op, M, N, K, ld_max)


def dense_f32_plan(op, M, N, K, ld_max=0):
    """(tile rows, tile columns, row slabs, workgroups) of a float32 dense launch (op: _lib.DENSE_F32_NT / _NN / _TN), or None
    where octic_dense_f32_plan refuses the problem."""
    return _dense_f32_query(int(op), operator.index(M), int(N), int(K), int(ld_max))


def dense_f32_ok(M, N, K, ld_max=0):
    """csrc/dense_f32.hip takes a linear layer with M rows, N = out_features, K = in_features in all three directions (forward,
    input gradient, weight gradient); ld_max: the largest operand row stride in elements, 0 = not known."""
    return all(dense_f32_plan(op, M, N, K, ld_max) is not None for op in (_lib.DENSE_F32_NT, _lib.DENSE_F32_NN, _lib.DENSE_F32_TN))


def _f32_rows(t, width, what):
    if t.dim() != 2 or t.dtype != torch.float32 or t.shape[1] != width or t.stride(1) != 1:
        raise ValueError(f"{what} must be float32 [rows, {width}] with unit column stride, got {tuple(t.shape)} {t.dtype}")
    _require_cuda(t)
    return t


def _ld(t):
    """Row stride handed to the library: a one-row tensor's stride is arbitrary in torch, its row length serves."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def dense_f32_nt(a, w, bias=None, gelu=False, out=None, h_out=None, name=None):
    """C[M,N] = a[M,K] @ w[N,K]^T (+ bias) in exact float32 on csrc/dense_f32.hip.  gelu: returns (H, C) with H the
    pre-activation and C = gelu(H) (erf).  out / h_out: 2-D destinations (any row stride the library takes)."""
    M, K = a.shape
    N = w.shape[0]
    _f32_rows(a, K, "dense_f32_nt: a"), _f32_rows(w, K, "dense_f32_nt: w")
    if bias is not None and not (bias.is_cuda and bias.dtype == torch.float32 and bias.shape == (N,) and bias.is_contiguous()):
        raise ValueError(f"dense_f32_nt: bias must be a contiguous float32 [{N}] tensor on the GPU")
    c = torch.empty((M, N), dtype=torch.float32, device=a.device) if out is None else _f32_rows(out, N, "dense_f32_nt: out")
    h = None
    if gelu:
        h = torch.empty((M, N), dtype=torch.float32, device=a.device) if h_out is None else _f32_rows(h_out, N, "dense_f32_nt: h_out")
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_f32_nt(_p(a), _p(w), _p(bias), M, N, K, _ld(a), _ld(w), _p(c), _ld(c), int(bool(gelu)),
                                   _p(h), _ld(h) if gelu else 0, _stream(a)))
    KERNEL_TIMER.stop(t, name or ("dense_f32_nt_gelu_kernel" if gelu else "dense_f32_nt_kernel"),
                      4 * (M * K + N * K + M * N * (2 if gelu else 1)), 2.0 * M * N * K)
    return (h, c) if gelu else c


def dense_f32_nn(g, w, out=None, name=None):
    """DX[M,K] = g[M,N] @ w[N,K] in exact float32 (w as stored)."""
    M, N = g.shape
    K = w.shape[1]
    _f32_rows(g, N, "dense_f32_nn: g"), _f32_rows(w, K, "dense_f32_nn: w")
    if w.shape[0] != N:
        raise ValueError("dense_f32_nn: g [M,N] and w [N,K] disagree on N")
    dx = torch.empty((M, K), dtype=torch.float32, device=g.device) if out is None else _f32_rows(out, K, "dense_f32_nn: out")
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_f32_nn(_p(g), _p(w), M, N, K, _ld(g), _ld(w), _p(dx), _ld(dx), _stream(g)))
    KERNEL_TIMER.stop(t, name or "dense_f32_nn_kernel", 4 * (M * N + N * K + M * K), 2.0 * M * N * K)
    return dx


def dense_f32_tn(g, x, out=None, want_colsum=False, workspace=None, name=None):
    """DW[N,K] = g[M,N]^T @ x[M,K] in exact float32, bitwise repeatable (row slabs summed in slab order); out: write it there
    (a gradient-bucket view).  want_colsum: returns (DW, db) with db[N] the column sums of g.  The workspace comes from torch's
    allocator per call (capturable) unless one is given."""
    M, N = g.shape
    K = x.shape[1]
    _f32_rows(g, N, "dense_f32_tn: g"), _f32_rows(x, K, "dense_f32_tn: x")
    if x.shape[0] != M:
        raise ValueError("dense_f32_tn: g [M,N] and x [M,K] disagree on M")
    dw = torch.empty((N, K), dtype=torch.float32, device=g.device) if out is None else _f32_rows(out, K, "dense_f32_tn: out")
    db = torch.empty(N, dtype=torch.float32, device=g.device) if want_colsum else None
    need = int(lib().octic_dense_f32_workspace_bytes(_lib.DENSE_F32_TN, M, N, K))
    if need < 0:
        check(need)
    ws = workspace if workspace is not None else torch.empty(need, dtype=torch.uint8, device=g.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_f32_tn(_p(g), _p(x), M, N, K, _ld(g), _ld(x), _p(dw), _ld(dw), _p(db), _p(ws),
                                   ws.numel() * ws.element_size(), _stream(g)))
    KERNEL_TIMER.stop(t, name or "dense_f32_tn_kernel", 4 * (M * N + M * K + N * K), 2.0 * M * N * K)
    return (dw, db) if want_colsum else dw


def dense_gelu_bwd_f32(h, g, want_colsum=True):
    """dh = gelu'(h) * g for float32 [..., d] (contiguous); also the column sums of dh (f32 [d]) when asked."""
    _require_cuda(h)
    d = h.shape[-1]
    rows = h.numel() // d
    if h.dtype != torch.float32 or g.dtype != torch.float32 or g.shape != h.shape or not (h.is_contiguous() and g.is_contiguous()):
        raise ValueError("dense_gelu_bwd_f32: h and g must be contiguous float32 tensors of one shape")
    dh = torch.empty_like(h)
    db = torch.empty(d, dtype=torch.float32, device=h.device) if want_colsum else None
    partials = torch.empty((lib().octic_dense_gelu_blocks(), d), dtype=torch.float32, device=h.device) if want_colsum else None
    t = KERNEL_TIMER.start()
    check(lib().octic_dense_gelu_bwd_f32(_p(h), _p(g), _p(dh), _p(partials), _p(db), rows, d, _stream(h)))
    KERNEL_TIMER.stop(t, "dense_gelu_bwd_f32_kernel", rows * d * 12)
    return dh, db


# ------------------------------------------------------------------------------------------ linear probe (csrc/probe.hip)
def probe_features(pairs, F):
    """pairs: the (patch tokens [B, P, D], class token [B, D]) tuples of get_intermediate_layers(..., return_class_token=True),
    at most 4; F: f32 [B, >= (n+1) D].  Writes F[:, :(n+1) D] = [cls ... | mean patch of the last pair]."""
    n = len(pairs)
    patch, cls0 = pairs[-1][0], pairs[0][1]
    _require_cuda(patch)
    B, P, D = patch.shape
    dtype = patch.dtype
    for p, c in pairs:
        if c.dtype != dtype or p.dtype != dtype or tuple(c.shape) != (B, D) or c.stride(1) != 1:
            raise ValueError("probe_features: class tokens must be [B, D] rows of one dtype")
    if patch.stride(2) != 1 or F.dtype != torch.float32 or F.stride(1) != 1 or F.shape[0] < B:
        raise ValueError("probe_features: patch tokens / F must have contiguous channels")
    cls = (ctypes.c_void_p * n)(*[c.data_ptr() for _, c in pairs])
    cls_ld = (ctypes.c_int64 * n)(*[c.stride(0) for _, c in pairs])
    t = KERNEL_TIMER.start()
    check(lib().octic_probe_features(cls, cls_ld, n, _p(patch), patch.stride(0), patch.stride(1), dt_code(dtype), B, P, D,
                                     _p(F), F.stride(0), _stream(patch)))
    KERNEL_TIMER.stop(t, f"probe_features_kernel<{_DTN[dtype]}>", B * D * (P + n) * patch.element_size() + 4 * B * (n + 1) * D)
    return F


def probe_forward(table, nheads, F, B, C, logits, sumK):
    t = KERNEL_TIMER.start()
    check(lib().octic_probe_forward(_p(table), nheads, _p(F), F.stride(0), B, C, _p(logits), _stream(F)))
    KERNEL_TIMER.stop(t, "probe_forward_kernel", 4 * (C * sumK + nheads * B * C), 2.0 * B * C * sumK)


def probe_ce(logits, labels, nheads, B, C, dlogits, rowloss, rowrank, loss_mean=None, loss_sum=None, topk=None):
    if labels.dtype != torch.int64 or not labels.is_contiguous() or labels.numel() != B:
        raise ValueError("probe_ce: labels must be a contiguous int64 tensor of B class indices")
    t = KERNEL_TIMER.start()
    check(lib().octic_probe_ce(_p(logits), _p(labels), nheads, B, C, _p(dlogits), _p(rowloss), _p(rowrank), _p(loss_mean),
                               _p(loss_sum), _p(topk), _stream(logits)))
    KERNEL_TIMER.stop(t, "probe_ce_kernel", 4 * nheads * B * C * (3 if dlogits is not None else 2))


def probe_sgd(table, nheads, total_ktiles, F, dlogits, B, C, lr, momentum, sumK):
    t = KERNEL_TIMER.start()
    check(lib().octic_probe_sgd(_p(table), nheads, total_ktiles, _p(F), F.stride(0), _p(dlogits), B, C, _p(lr),
                                float(momentum), _stream(F)))
    KERNEL_TIMER.stop(t, "probe_sgd_kernel", 16 * C * sumK, 2.0 * B * C * sumK)


# ------------------------------------------------------------------------------------------ attentive probe (csrc/attnpool.hip)
# Thin launches: tensors are f32 on the GPU, `*_ptrs` are int64 device tensors of G per-classifier addresses (ptr_table below);
# the library refuses bad shapes and alignments.  Names ending in _mfma are GEMM-shaped (bench_attnpool bounds them by the f32
# MFMA rate, the others by HBM).
def ptr_table(tensors, device):
    """Device array of the tensors' addresses (int64), the `const float* const*` of the attnpool entry points."""
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=device)


def attnpool_fold(q_ptrs, wk_ptrs, G, D, U):
    _require_cuda(U)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_fold(_p(q_ptrs), _p(wk_ptrs), G, D, _p(U), U.shape[0], _stream(U)))
    KERNEL_TIMER.stop(t, "attnpool_fold_kernel", 4 * (G * D * D + G * D + U.numel()))


def attnpool_softmax(S, B, N, GH):
    _require_cuda(S)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_softmax(_p(S), S.stride(0), B, N, GH, _stream(S)))
    KERNEL_TIMER.stop(t, "attnpool_softmax_kernel", 4 * 4 * S.numel())


def attnpool_pool(P, X, ldx, B, N, D, GH, Z):
    _require_cuda(X)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_pool(_p(P), P.stride(0), _p(X), ldx, B, N, D, GH, _p(Z), _stream(X)))
    KERNEL_TIMER.stop(t, "attnpool_pool_mfma", 4 * B * (N * GH + N * D + GH * D), 2.0 * B * N * GH * D)


def attnpool_value(Z, wv_ptrs, bv_ptrs, B, G, D, pooled):
    _require_cuda(Z)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_value(_p(Z), _p(wv_ptrs), _p(bv_ptrs), B, G, D, _p(pooled), pooled.stride(0), _stream(Z)))
    KERNEL_TIMER.stop(t, "attnpool_value_mfma", 4 * (B * G * D * (D // 64 + 1) + G * D * D), 2.0 * B * G * D * D)


def attnpool_dinput(dlogits, w_ptrs, G, B, C, D, alpha, dF):
    _require_cuda(dlogits)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_dinput(_p(dlogits), _p(w_ptrs), G, B, C, D, float(alpha), _p(dF), dF.stride(0), _stream(dF)))
    KERNEL_TIMER.stop(t, "attnpool_dinput_mfma", 4 * G * (B * C + C * D + B * D), 2.0 * G * B * C * D)


def attnpool_dweight(dlogits, F, col0, col_stride, G, B, C, K, alpha, dw_ptrs):
    _require_cuda(dlogits)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_dweight(_p(dlogits), _p(F), F.stride(0), col0, col_stride, G, B, C, K, float(alpha), _p(dw_ptrs),
                                       _stream(F)))
    KERNEL_TIMER.stop(t, "attnpool_dweight_mfma", 4 * G * (B * C + B * K + C * K), 2.0 * G * B * C * K)


def attnpool_colsum(src, group_stride, ld, G, rows, cols, alpha, dst_ptrs):
    _require_cuda(src)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_colsum(_p(src), group_stride, ld, G, rows, cols, float(alpha), _p(dst_ptrs), _stream(src)))
    KERNEL_TIMER.stop(t, "attnpool_colsum_kernel", 4 * G * cols * (rows + 1))


def attnpool_dz(dpooled, wv_ptrs, B, G, D, dZ):
    _require_cuda(dpooled)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_dz(_p(dpooled), dpooled.stride(0), _p(wv_ptrs), B, G, D, _p(dZ), _stream(dZ)))
    KERNEL_TIMER.stop(t, "attnpool_dz_mfma", 4 * (B * G * D * (D // 64 + 1) + G * D * D), 2.0 * B * G * D * D)


def attnpool_dwv(dpooled, Z, B, G, D, dwv_ptrs):
    _require_cuda(dpooled)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_dwv(_p(dpooled), dpooled.stride(0), _p(Z), B, G, D, _p(dwv_ptrs), _stream(Z)))
    KERNEL_TIMER.stop(t, "attnpool_dwv_mfma", 4 * (B * G * D * (D // 64 + 1) + G * D * D), 2.0 * B * G * D * D)


def attnpool_dscores(X, ldx, dZ, P, B, N, D, GH, dS):
    _require_cuda(X)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_dscores(_p(X), ldx, _p(dZ), _p(P), P.stride(0), B, N, D, GH, _p(dS), _stream(X)))
    KERNEL_TIMER.stop(t, "attnpool_dscores_mfma", 4 * B * (N * D + GH * D + 4 * N * GH), 2.0 * B * N * GH * D)


def attnpool_unfold(q_ptrs, wk_ptrs, dU, G, D, dq_ptrs, dwk_ptrs, dbk_ptrs):
    _require_cuda(dU)
    t = KERNEL_TIMER.start()
    check(lib().octic_attnpool_unfold(_p(q_ptrs), _p(wk_ptrs), _p(dU), G, D, _p(dq_ptrs), _p(dwk_ptrs), _p(dbk_ptrs), _stream(dU)))
    KERNEL_TIMER.stop(t, "attnpool_unfold_kernel", 4 * (2 * G * D * D + G * D * (D // 64) + 3 * G * D))


# ------------------------------------------------------------------------------------------ segmentation logreg (csrc/segeval.hip)
def _seg_rows(X):
    """X as f32 rows: [N, D] with contiguous channels and a 16-byte aligned row stride."""
    _require_cuda(X)
    if X.dim() != 2 or X.dtype != torch.float32 or X.stride(1) != 1:
        raise ValueError("segmentation ops take an f32 [N, D] matrix with contiguous channels")
    return X.shape[0], X.shape[1], X.stride(0)


def seg_ldd(C):
    """Row stride (floats) of the dlogits buffer for C classes: 32 ceil(C / 32)."""
    ldd = lib().octic_seg_ldd(int(C))
    check(min(ldd, 0))
    return ldd


def seg_workspace(N, D, C, device):
    """The workspace of seg_value_dlogits / seg_wgrad for this shape (loss partials, slab tiles)."""
    nbytes = lib().octic_seg_workspace_bytes(N, D, C)
    check(min(nbytes, 0))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def seg_value_dlogits(X, W, b, y, dlogits, value, workspace):
    """value[0] (f64) = sum_n CE(X_n W^T + b, y_n); dlogits [N, seg_ldd(C)] = softmax - onehot.  y: int32 class indices."""
    N, D, ldx = _seg_rows(X)
    C = W.shape[0]
    if (W.dtype != torch.float32 or not W.is_contiguous() or W.shape[1] != D or b.dtype != torch.float32 or b.numel() != C
            or not b.is_contiguous()):
        raise ValueError("seg_value_dlogits: W must be a contiguous f32 [C, D], b a contiguous f32 [C]")
    if y.dtype != torch.int32 or not y.is_contiguous() or y.numel() != N:
        raise ValueError("seg_value_dlogits: y must be a contiguous int32 tensor of N class indices")
    if (dlogits.dtype != torch.float32 or not dlogits.is_contiguous() or dlogits.numel() < N * max(seg_ldd(C), 0)
            or value.dtype != torch.float64):
        raise ValueError("seg_value_dlogits: dlogits must be a contiguous f32 [N, seg_ldd(C)], value an f64 scalar")
    t = KERNEL_TIMER.start()
    check(lib().octic_seg_value_dlogits(_p(X), ldx, N, D, _p(W), _p(b), C, _p(y), _p(dlogits), _p(value), _p(workspace),
                                        _stream(X)))
    KERNEL_TIMER.stop(t, "seg_forward_kernel", 4 * N * (D + seg_ldd(C)), 2.0 * N * C * D)


def seg_predict(X, W, b, pred):
    """pred[n] (int32) = argmax_c (X_n W^T + b)_c, the first maximum."""
    N, D, ldx = _seg_rows(X)
    C = W.shape[0]
    if W.dtype != torch.float32 or not W.is_contiguous() or W.shape[1] != D or b.dtype != torch.float32 or b.numel() != C:
        raise ValueError("seg_predict: W must be a contiguous f32 [C, D], b an f32 [C]")
    if pred.dtype != torch.int32 or not pred.is_contiguous() or pred.numel() != N:
        raise ValueError("seg_predict: pred must be a contiguous int32 [N]")
    t = KERNEL_TIMER.start()
    check(lib().octic_seg_predict(_p(X), ldx, N, D, _p(W), _p(b), C, _p(pred), _stream(X)))
    KERNEL_TIMER.stop(t, "seg_forward_kernel<predict>", 4 * N * (D + 1), 2.0 * N * C * D)


def seg_wgrad(X, dlogits, W, scale, lam, dW, db, workspace):
    """dW = scale dlogits^T X + lam W, db = scale colsum(dlogits) (f32 [C, D] / [C])."""
    N, D, ldx = _seg_rows(X)
    C = W.shape[0]
    if (dW.dtype != torch.float32 or not dW.is_contiguous() or tuple(dW.shape) != (C, D) or db.dtype != torch.float32
            or db.numel() != C or not W.is_contiguous() or W.dtype != torch.float32):
        raise ValueError("seg_wgrad: W / dW must be contiguous f32 [C, D], db an f32 [C]")
    t = KERNEL_TIMER.start()
    check(lib().octic_seg_wgrad(_p(X), ldx, N, D, _p(dlogits), C, _p(W), float(scale), float(lam), _p(dW), _p(db),
                                _p(workspace), _stream(X)))
    KERNEL_TIMER.stop(t, "seg_wgrad_kernel", 4 * N * D, 2.0 * N * C * D)


def seg_colstats(X):
    """(mean, var): f64 [D] column mean and population variance of the f32 rows X [N, D]."""
    N, D, ldx = _seg_rows(X)
    nbytes = lib().octic_seg_colstats_workspace_bytes(N, D)
    check(min(nbytes, 0))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=X.device)
    mean = torch.empty(D, dtype=torch.float64, device=X.device)
    var = torch.empty(D, dtype=torch.float64, device=X.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_seg_colstats(_p(X), ldx, N, D, _p(mean), _p(var), _p(ws), _stream(X)))
    KERNEL_TIMER.stop(t, "seg_colstats_kernel", 4 * N * D)
    return mean, var


def seg_standardize_(X, mean, scale):
    """In place: x = float(float(x - mean) / scale) with f64 [D] mean and scale."""
    N, D, ldx = _seg_rows(X)
    for v in (mean, scale):
        if v.dtype != torch.float64 or v.numel() != D or not v.is_contiguous() or v.device != X.device:
            raise ValueError("seg_standardize_: mean and scale must be contiguous f64 [D] on X's device")
    t = KERNEL_TIMER.start()
    check(lib().octic_seg_standardize(_p(X), ldx, N, D, _p(mean), _p(scale), _stream(X)))
    KERNEL_TIMER.stop(t, "seg_standardize_kernel", 8 * N * D)
    return X


_SEG_LABEL_DTYPES = (torch.uint8, torch.int16, torch.int32, torch.int64)


def _seg_labels(labels):
    _require_cuda(labels)
    if labels.dim() != 2 or labels.dtype not in _SEG_LABEL_DTYPES or not labels.is_contiguous():
        raise ValueError("segmentation labels must be a contiguous [R, L] tensor of uint8 / int16 / int32 / int64 values 0 .. 255")
    return labels.shape[0], labels.shape[1], labels.element_size()


def seg_patch_mode(labels):
    """mode[r] (int32) = the most frequent value of labels[r, :], the smallest on a tie (torch.mode)."""
    R, L, es = _seg_labels(labels)
    mode = torch.empty(R, dtype=torch.int32, device=labels.device)
    if R:
        t = KERNEL_TIMER.start()
        check(lib().octic_seg_patch_mode(_p(labels), es, R, L, _p(mode), _stream(labels)))
        KERNEL_TIMER.stop(t, "seg_mode_kernel", R * (L * es + 4))
    return mode


def seg_confusion(labels, pred, ignore, counts):
    """counts[t, pred[r]] += pixels of row r with label t, for every t with ignore[t] == 0 (uint8 [256]); counts: int64
    [256, 256], accumulated."""
    R, L, es = _seg_labels(labels)
    if (pred.dtype != torch.int32 or pred.numel() != R or not pred.is_contiguous() or ignore.dtype != torch.uint8
            or ignore.numel() != 256 or counts.dtype != torch.int64 or counts.numel() != 65536 or not counts.is_contiguous()):
        raise ValueError("seg_confusion: pred int32 [R], ignore uint8 [256], counts int64 [256, 256]")
    if R:
        t = KERNEL_TIMER.start()
        check(lib().octic_seg_confusion(_p(labels), es, R, L, _p(pred), _p(ignore), _p(counts), _stream(labels)))
        KERNEL_TIMER.stop(t, "seg_confusion_kernel", R * (L * es + 4))
    return counts


# ------------------------------------------------------------------------------------------ the two k-NN searches (csrc/knn_common.hpp)
def _knn_workspace(nbytes, device):
    """The workspace of the byte count that a *_workspace_bytes query answered (a negative answer is its error code)."""
    check(min(nbytes, 0))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _knn_out_ok(o, dtype, n, kmax, ldo, device):
    """o is a ``dtype`` [n, >= kmax] tensor of rows with stride ldo on ``device``."""
    return (o.dtype == dtype and o.dim() == 2 and o.shape[0] == n and o.shape[1] >= kmax and o.stride(1) == 1 and o.stride(0) == ldo
            and o.device == device)


def _knn_stream_bytes(plan, n, M, D):
    """Algorithmic bytes of the plan's tiles: every workgroup streams its share of the keys once per query tile, the queries
    once per key tile."""
    _, qt, kt, _ = plan
    return 4 * D * (M * ((n + qt - 1) // qt) + n * ((M + kt - 1) // kt))


# ------------------------------------------------------------------------------------------ segmentation k-NN (csrc/segknn.hip)
KNN_L2, KNN_COSINE, KNN_BOTH = 1, 2, 3
KNN_KMAX = 32


def seg_knn_plan(n, M, D, kmax, metrics=KNN_BOTH):
    """octic_seg_knn_plan: (key-axis splits, query rows per tile, keys per tile, workspace class)."""
    answer = _lib.plan("octic_seg_knn_plan", int(n), int(M), int(D), int(kmax), int(metrics))
    if answer is None:
        check(-1)
    return answer


def seg_knn_workspace(n, M, D, kmax, metrics, splits, device):
    """The workspace of seg_knn for this shape and split count (0 = the plan's): the partial lists of the splits."""
    return _knn_workspace(lib().octic_seg_knn_workspace_bytes(n, M, D, kmax, metrics, splits), device)


_KNN_ROW_DTYPES = {torch.float32: ("", "f32"), torch.bfloat16: ("_bf16", "bf16")}   # entry-point suffix, KERNEL_TIMER tag


def _seg_knn_rows(X):
    """X as the rows of the k-NN search: f32 or bf16 [N, D] with contiguous channels -> (N, D, row stride, suffix, tag)."""
    _require_cuda(X)
    if X.dim() != 2 or X.dtype not in _KNN_ROW_DTYPES or X.stride(1) != 1:
        raise ValueError("the segmentation k-NN ops take an f32 or bf16 [N, D] matrix with contiguous channels")
    return (X.shape[0], X.shape[1], X.stride(0)) + _KNN_ROW_DTYPES[X.dtype]


def seg_rownorms(X):
    """f32 [N]: the squared norm of every row of the f32 or bf16 rows X [N, D], summed in f32 in a fixed order."""
    N, D, ldx, suffix, tag = _seg_knn_rows(X)
    norms = torch.empty(N, dtype=torch.float32, device=X.device)
    t = KERNEL_TIMER.start()
    check(getattr(lib(), "octic_seg_rownorms" + suffix)(_p(X), ldx, N, D, _p(norms), _stream(X)))
    KERNEL_TIMER.stop(t, f"seg_rownorms_kernel<{tag}>", X.element_size() * N * D + 4 * N, 2.0 * N * D)
    return norms


def seg_knn(Q, K, qnorm, knorm, skip, kmax, metrics=KNN_BOTH, splits=0, out=None, workspace=None):
    """The kmax nearest rows of K for every row of Q under the squared L2 distance (metrics & 1), the cosine distance
    (metrics & 2) or both, ordered by (distance, key row index).  skip: None or uint8 [M], non-zero = the key is never listed.
    Q and K are both f32 or both bf16 rows (bf16: values rounded once by the caller; everything after is f32, see
    include/octic_hip.h); a mixed pair is a ValueError.
    Returns (idx_l2, dist_l2, idx_cos, dist_cos): int32 / f32 [n, kmax], None for a metric not asked for.  ``out`` may hold
    those four as 2-d tensors with a common row stride >= kmax (columns past kmax are left alone)."""
    if K.dtype != Q.dtype:
        raise ValueError(f"seg_knn: Q ({Q.dtype}) and K ({K.dtype}) must share one dtype")
    n, D, ldq, suffix, tag = _seg_knn_rows(Q)
    M, Dk, ldk, _, _ = _seg_knn_rows(K)
    if Dk != D or K.device != Q.device:
        raise ValueError("seg_knn: Q and K must have the same width and device")
    for v, rows in ((qnorm, n), (knorm, M)):
        if v.dtype != torch.float32 or v.numel() != rows or not v.is_contiguous() or v.device != Q.device:
            raise ValueError("seg_knn: qnorm / knorm must be contiguous f32 [n] / [M] on the device of Q")
    if skip is not None and (skip.dtype != torch.uint8 or skip.numel() != M or not skip.is_contiguous() or skip.device != Q.device):
        raise ValueError("seg_knn: skip must be a contiguous uint8 [M] on the device of Q")
    if metrics not in (KNN_L2, KNN_COSINE, KNN_BOTH):
        raise ValueError("seg_knn: metrics must be KNN_L2, KNN_COSINE or KNN_BOTH")
    if not 1 <= kmax <= KNN_KMAX:
        raise ValueError(f"seg_knn: kmax must be in 1 .. {KNN_KMAX}")
    if out is None:
        out = [torch.empty(n, kmax, dtype=dt, device=Q.device) if metrics & bit else None
               for bit in (KNN_L2, KNN_COSINE) for dt in (torch.int32, torch.float32)]
    given = [o for o in out if o is not None]
    ldo = given[0].stride(0)
    for o, dt, bit in zip(out, (torch.int32, torch.float32) * 2, (KNN_L2, KNN_L2, KNN_COSINE, KNN_COSINE)):
        if o is None:
            if metrics & bit:
                raise ValueError("seg_knn: out lacks a tensor of a metric that is asked for")
            continue
        if not _knn_out_ok(o, dt, n, kmax, ldo, Q.device):
            raise ValueError("seg_knn: out tensors must be int32 / f32 [n, >= kmax] rows with one common row stride")
    if workspace is None:
        workspace = seg_knn_workspace(n, M, D, kmax, metrics, splits, Q.device)
    t = KERNEL_TIMER.start()
    check(getattr(lib(), "octic_seg_knn" + suffix)(_p(Q), ldq, n, _p(K), ldk, M, D, _p(qnorm), _p(knorm), _p(skip), kmax, metrics,
                                                   splits, *[_p(o) for o in out], ldo, _p(workspace), _stream(Q)))
    nl = 2 if metrics == KNN_BOTH else 1
    stream_bytes = _knn_stream_bytes(seg_knn_plan(n, M, D, kmax, metrics), n, M, D) * Q.element_size() // 4
    KERNEL_TIMER.stop(t, f"seg_knn_kernel<{tag}, {metrics}>", stream_bytes + 8 * nl * n * kmax, 2.0 * n * M * D)
    return tuple(out)


def seg_knn_vote(idx, labels, ks, out=None):
    """uint8 [len(ks), n, L]: per query row and pixel the most frequent of labels[idx[row, :k], pixel] for every k of the
    ascending ``ks`` (at most 8 values <= 32), the smallest value on a tie (torch.mode)."""
    R, L, es = _seg_labels(labels)
    ks = [int(k) for k in ks]
    if (idx.dtype != torch.int32 or idx.dim() != 2 or idx.stride(1) != 1 or idx.device != labels.device or not ks
            or len(ks) > 8 or idx.shape[1] < ks[-1]):
        raise ValueError("seg_knn_vote: idx must be int32 [n, >= max(ks)] rows on the device of labels, ks 1 .. 8 values")
    n = idx.shape[0]
    if out is None:
        out = torch.empty(len(ks), n, L, dtype=torch.uint8, device=labels.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (len(ks), n, L) or not out.is_contiguous() or out.device != labels.device:
        raise ValueError("seg_knn_vote: out must be a contiguous uint8 [len(ks), n, L]")
    if n:
        t = KERNEL_TIMER.start()
        check(lib().octic_seg_knn_vote(_p(idx), idx.stride(0), n, _p(labels), es, R, L, (ctypes.c_int * len(ks))(*ks), len(ks),
                                       _p(out), _stream(labels)))
        KERNEL_TIMER.stop(t, "seg_knn_vote_kernel", n * (4 * ks[-1] + L * (es * ks[-1] + len(ks))))
    return out


# ------------------------------------------------------------------------------------------ classification k-NN (csrc/knn_cls.hip)
KNN_CLS_KMAX = 256             # OCTIC_KNN_KMAX of include/octic_hip.h


def knn_topk_plan(n, M, D, kmax):
    """octic_knn_topk_plan: (key-axis splits, query rows per tile, keys per tile, workspace class)."""
    answer = _lib.plan("octic_knn_topk_plan", int(n), int(M), int(D), int(kmax))
    if answer is None:
        check(-1)
    return answer


def knn_topk_workspace(n, M, D, kmax, splits, device):
    """The workspace of knn_topk for this shape and split count (0 = the plan's): the partial lists of the splits."""
    return _knn_workspace(lib().octic_knn_topk_workspace_bytes(n, M, D, kmax, splits), device)


def knn_topk(Q, K, kmax, splits=0, out=None, workspace=None):
    """The kmax rows of K with the largest inner product for every row of Q, ordered by (similarity descending, key row index
    ascending).  Returns (idx int32, sim f32), both [n, kmax].  ``out`` may hold the two as 2-d tensors with a common row
    stride >= kmax (columns past kmax are left alone)."""
    n, D, ldq = _seg_rows(Q)
    M, Dk, ldk = _seg_rows(K)
    if Dk != D or K.device != Q.device:
        raise ValueError("knn_topk: Q and K must have the same width and device")
    if not 1 <= kmax <= KNN_CLS_KMAX:
        raise ValueError(f"knn_topk: kmax must be in 1 .. {KNN_CLS_KMAX}")
    if out is None:
        out = (torch.empty(n, kmax, dtype=torch.int32, device=Q.device), torch.empty(n, kmax, dtype=torch.float32, device=Q.device))
    idx, sim = out
    ldo = idx.stride(0)
    for o, dt in ((idx, torch.int32), (sim, torch.float32)):
        if not _knn_out_ok(o, dt, n, kmax, ldo, Q.device):
            raise ValueError("knn_topk: out must be (int32, f32) [n, >= kmax] rows with one common row stride")
    if workspace is None:
        workspace = knn_topk_workspace(n, M, D, kmax, splits, Q.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_knn_topk(_p(Q), ldq, n, _p(K), ldk, M, D, kmax, splits, _p(idx), _p(sim), ldo, _p(workspace), _stream(Q)))
    KERNEL_TIMER.stop(t, "knn_topk_kernel", _knn_stream_bytes(knn_topk_plan(n, M, D, kmax), n, M, D) + 8 * n * kmax, 2.0 * n * M * D)
    return idx, sim


def knn_vote(sim, idx, labels, num_classes, inv_T, ks, out=None, targets=None, counters=None):
    """f32 [len(ks), n, C]: probas[i, r, c] = the sum over j < ks[i] with labels[idx[r, j]] == c of softmax(sim[r] * inv_T)[j],
    the softmax over all kmax = sim.shape[1] entries.  ks: 1 .. 8 strictly ascending values <= kmax.  With ``targets`` (int64 [n])
    and ``counters`` (int64 [len(ks), 2]) the launch adds each k's top-1 / top-5 hits to the counters."""
    _require_cuda(sim)
    ks = [int(k) for k in ks]
    C = int(num_classes)
    if (sim.dtype != torch.float32 or idx.dtype != torch.int32 or sim.dim() != 2 or idx.shape != sim.shape or sim.stride(1) != 1
            or idx.stride(1) != 1 or idx.stride(0) != sim.stride(0) or idx.device != sim.device):
        raise ValueError("knn_vote: sim f32 / idx int32 must be [n, kmax] rows with one common row stride on one device")
    n, kmax = sim.shape
    if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous() or labels.device != sim.device:
        raise ValueError("knn_vote: labels must be a contiguous int64 [M] on the device of sim")
    if not ks or len(ks) > 8 or not 1 <= kmax <= KNN_CLS_KMAX:
        raise ValueError(f"knn_vote: 1 .. 8 values of k, kmax in 1 .. {KNN_CLS_KMAX}")
    if (targets is None) != (counters is None):
        raise ValueError("knn_vote: targets and counters go together")
    if targets is not None and (targets.dtype != torch.int64 or targets.numel() != n or not targets.is_contiguous()
                                or targets.device != sim.device or counters.dtype != torch.int64
                                or tuple(counters.shape) != (len(ks), 2) or not counters.is_contiguous()
                                or counters.device != sim.device):
        raise ValueError("knn_vote: targets int64 [n] and counters int64 [len(ks), 2], contiguous, on the device of sim")
    if out is None:
        out = torch.empty(len(ks), n, C, dtype=torch.float32, device=sim.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (len(ks), n, C) or not out.is_contiguous() or out.device != sim.device:
        raise ValueError("knn_vote: out must be a contiguous f32 [len(ks), n, C]")
    if n:
        t = KERNEL_TIMER.start()
        check(lib().octic_knn_vote(_p(sim), _p(idx), sim.stride(0), n, kmax, _p(labels), labels.numel(), C, float(inv_T),
                                   (ctypes.c_int * len(ks))(*ks), len(ks), _p(out), _p(targets), _p(counters), _stream(sim)))
        KERNEL_TIMER.stop(t, "knn_vote_kernel", n * (16 * kmax + 4 * len(ks) * C))
    return out


# ------------------------------------------------------------------------------------------ top-k accuracy counters (csrc/topk_metric.hip)
TOPK_MAX_TARGETS = 32          # OCTIC_TOPK_MAX_TARGETS of include/octic_hip.h
TOPK_ANY, TOPK_CLASS = 0, 1    # OCTIC_TOPK_ANY / OCTIC_TOPK_CLASS
TOPK_ORDER_STRICT, TOPK_ORDER_INDEX = 0, 1


def topk_shapes(scores, targets):
    """(G, n, C, A) of a scores [n, C] | [G, n, C] / targets [n] | [n, A] pair; raises ValueError for anything else.  Looks at
    shapes only, so it runs on CPU tensors too."""
    if scores.dim() not in (2, 3) or targets.dim() not in (1, 2):
        raise ValueError("topk metric: scores must be [n, C] or [G, n, C] and targets [n] or [n, A]")
    G = scores.shape[0] if scores.dim() == 3 else 1
    n, C = scores.shape[-2], scores.shape[-1]
    A = targets.shape[1] if targets.dim() == 2 else 1
    if targets.shape[0] != n:
        raise ValueError(f"topk metric: {targets.shape[0]} target rows for {n} score rows")
    if not 1 <= A <= TOPK_MAX_TARGETS:
        raise ValueError(f"topk metric: 1 .. {TOPK_MAX_TARGETS} targets per row, got {A}")
    if C < 1 or G * n * A >= 2 ** 31 or C >= 2 ** 31:
        raise ValueError("topk metric: at least one column, and groups * rows * targets and columns below 2^31")
    return G, n, C, A


def topk_rank(scores, targets, class_map=None, order=TOPK_ORDER_STRICT, out=None):
    """int32 [G, n, A]: for every target the number of candidates that come before it among the row's candidates
    ``scores[g, r, class_map[j]]`` (class_map None: all C columns), Cm for a target outside [0, Cm).  scores f32 [n, C] or
    [G, n, C] with unit column stride (any row / group stride: no copy), targets int64 [n] or [n, A] contiguous, class_map a
    contiguous int32 [Cm] on the device whose entries the CALLER has checked to lie in [0, C).  order: TOPK_ORDER_STRICT (a score
    strictly greater comes before) or TOPK_ORDER_INDEX (... or an equal score at a lower candidate index)."""
    G, n, C, A = topk_shapes(scores, targets)
    _require_cuda(scores)
    if scores.dtype != torch.float32 or scores.stride(-1) != 1:
        raise ValueError("topk_rank: scores must be f32 with unit column stride")
    if targets.dtype != torch.int64 or not targets.is_contiguous() or targets.device != scores.device:
        raise ValueError("topk_rank: targets must be a contiguous int64 tensor on the device of scores")
    Cm = C
    if class_map is not None:
        if class_map.dtype != torch.int32 or class_map.dim() != 1 or not class_map.is_contiguous() or class_map.device != scores.device \
                or not class_map.numel():
            raise ValueError("topk_rank: class_map must be a contiguous, non-empty int32 [Cm] on the device of scores")
        Cm = class_map.numel()
    if order not in (TOPK_ORDER_STRICT, TOPK_ORDER_INDEX):
        raise ValueError("topk_rank: order is TOPK_ORDER_STRICT or TOPK_ORDER_INDEX")
    if out is None:
        out = torch.empty(G, n, A, dtype=torch.int32, device=scores.device)
    elif out.dtype != torch.int32 or tuple(out.shape) != (G, n, A) or not out.is_contiguous() or out.device != scores.device:
        raise ValueError("topk_rank: out must be a contiguous int32 [G, n, A]")
    if n:
        ld_r = scores.stride(-2) if n > 1 else C
        ld_g = scores.stride(0) if scores.dim() == 3 and G > 1 else n * max(ld_r, C)
        t = KERNEL_TIMER.start()
        check(lib().octic_topk_rank(_p(scores), ld_g, ld_r, G, n, C, _p(class_map), Cm, _p(targets), A, order, _p(out),
                                    _stream(scores)))
        KERNEL_TIMER.stop(t, "topk_rank_kernel", G * n * (4 * Cm + 4 * A) + 8 * n * A + (4 * Cm if class_map is not None else 0))
    return out


def topk_count(rank, counters, ks, mode=TOPK_ANY, num_classes=None, targets=None):
    """Adds the ranks of one update (int32 [G, n, A] of topk_rank over num_classes candidates) to the int64 device counters:
    TOPK_ANY [G, 1 + len(ks)] (rows with a defined target, then rows with a rank below each k), TOPK_CLASS [G, num_classes,
    1 + len(ks)] (per target class; A == 1, targets as given to topk_rank).  ks: 1 .. 8 strictly ascending values >= 1."""
    _require_cuda(rank)
    ks = [int(k) for k in ks]
    if rank.dtype != torch.int32 or rank.dim() != 3 or not rank.is_contiguous():
        raise ValueError("topk_count: rank must be a contiguous int32 [G, n, A]")
    G, n, A = rank.shape
    Cm = int(num_classes)
    if not ks or len(ks) > 8 or ks[0] < 1 or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("topk_count: ks must be 1 .. 8 strictly ascending values >= 1")
    want = (G, 1 + len(ks)) if mode == TOPK_ANY else (G, Cm, 1 + len(ks))
    if counters.dtype != torch.int64 or tuple(counters.shape) != want or not counters.is_contiguous() or counters.device != rank.device:
        raise ValueError(f"topk_count: counters must be a contiguous int64 {list(want)} on the device of rank")
    if mode == TOPK_CLASS:
        if A != 1:
            raise ValueError("topk_count: per-class counters take one target per row")
        if targets is None or targets.dtype != torch.int64 or targets.numel() != n or not targets.is_contiguous() \
                or targets.device != rank.device:
            raise ValueError("topk_count: per-class counters need the contiguous int64 [n] targets on the device of rank")
    elif mode != TOPK_ANY:
        raise ValueError("topk_count: mode is TOPK_ANY or TOPK_CLASS")
    if n:
        t = KERNEL_TIMER.start()
        check(lib().octic_topk_count(_p(rank), G, n, A, Cm, _p(targets if mode == TOPK_CLASS else None), mode,
                                     (ctypes.c_int * len(ks))(*ks), len(ks), _p(counters), _stream(rank)))
        KERNEL_TIMER.stop(t, "topk_count_kernel", 4 * G * n * A)


# ------------------------------------------------------------------------------------------ Mixup / CutMix + BCE (csrc/mixup.hip)
def _mix_table(table, B):
    _require_cuda(table)
    if table.dtype != torch.int32 or tuple(table.shape) != (B, 8) or not table.is_contiguous():
        raise ValueError(f"mix ops: the parameter table must be a contiguous int32 [{B}, 8] tensor (MixParams.table())")
    return table


def _mix_labels(labels, B=None):
    _require_cuda(labels)
    if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous() or (B is not None and labels.numel() != B):
        raise ValueError("mix ops: labels must be a contiguous int64 tensor of B class indices")
    return labels


def mix_images(src, table, dst):
    """dst = the batch src [B, C, H, W] (f32, contiguous) mixed as the device table says; out of place."""
    _require_cuda(src)
    _require_cuda(dst)
    if src.dim() != 4 or src.dtype != torch.float32 or not src.is_contiguous():
        raise ValueError("mix_images: images must be a contiguous f32 [B, C, H, W] tensor")
    if dst.shape != src.shape or dst.dtype != torch.float32 or not dst.is_contiguous():
        raise ValueError("mix_images: the output must be a contiguous f32 tensor of the images' shape")
    B, C, H, W = src.shape
    _mix_table(table, B)
    t = KERNEL_TIMER.start()
    check(lib().octic_mix_images(_p(src), _p(dst), _p(table), B, C, H, W, _stream(src)))
    KERNEL_TIMER.stop(t, "mix_images_kernel", 12 * src.numel())
    return dst


def mix_targets(labels, table, num_classes, on, off, binarize, targets, row0=0):
    """targets [rows, num_classes] f32 for the batch rows row0 .. row0 + rows - 1."""
    _require_cuda(targets)
    B = _mix_labels(labels).numel()
    _mix_table(table, B)
    if targets.dtype != torch.float32 or targets.dim() != 2 or targets.shape[1] != num_classes or not targets.is_contiguous():
        raise ValueError("mix_targets: the output must be a contiguous f32 [rows, num_classes] tensor")
    t = KERNEL_TIMER.start()
    check(lib().octic_mix_targets(_p(labels), _p(table), B, int(row0), targets.shape[0], int(num_classes), float(on), float(off),
                                  int(bool(binarize)), _p(targets), _stream(labels)))
    KERNEL_TIMER.stop(t, "mix_targets_kernel", 4 * targets.numel())
    return targets


def mix_bce(logits, labels, table, on, off, binarize, row0=0, loss=None, workspace=None, gscale=None, dlogits=None):
    """BCEWithLogitsLoss(mean) of logits [rows, num_classes] (f32 / bf16, unit column stride) against the mixed targets of the
    batch rows row0 ..: loss (f32 scalar, with workspace = rows f64) and / or dlogits (the logits' dtype) scaled by gscale."""
    _require_cuda(logits)
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError("mix_bce: logits must be [rows, num_classes] with contiguous columns")
    rows, nc = logits.shape
    B = _mix_labels(labels).numel()
    _mix_table(table, B)
    if dlogits is not None and (dlogits.dtype != logits.dtype or dlogits.shape != logits.shape or dlogits.stride(1) != 1):
        raise ValueError("mix_bce: dlogits must have the logits' shape and dtype")
    if loss is not None and (loss.dtype != torch.float32 or workspace is None or workspace.dtype != torch.float64
                             or workspace.numel() < rows):
        raise ValueError("mix_bce: the loss is an f32 scalar and needs a workspace of rows f64")
    t = KERNEL_TIMER.start()
    check(lib().octic_mix_bce(_p(logits), dt_code(logits.dtype), logits.stride(0), _p(labels), _p(table), B, int(row0), rows, nc,
                              float(on), float(off), int(bool(binarize)), _p(loss), _p(gscale), _p(dlogits),
                              dlogits.stride(0) if dlogits is not None else 0, _p(workspace), _stream(logits)))
    KERNEL_TIMER.stop(t, f"mix_bce_kernel<{_DTN[logits.dtype]}>", logits.numel() * logits.element_size() * (2 if dlogits is not None else 1))


def _criterion_args(what, logits, logit_rows, rows, labels, table, loss, workspace, dlogits):
    _require_cuda(logits)
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] != logit_rows:
        raise ValueError(f"{what}: logits must be [{logit_rows}, num_classes] with contiguous columns")
    B = _mix_labels(labels).numel()
    _mix_table(table, B)
    if dlogits is not None and (dlogits.dtype != logits.dtype or dlogits.shape != logits.shape or dlogits.stride(1) != 1):
        raise ValueError(f"{what}: dlogits must have the logits' shape and dtype")
    if loss is not None and (loss.dtype != torch.float32 or workspace is None or workspace.dtype != torch.float64
                             or workspace.numel() < rows):
        raise ValueError(f"{what}: the loss is an f32 scalar and needs a workspace of rows f64")
    return B


def mix_ce(logits, labels, table, on, off, row0=0, loss=None, workspace=None, gscale=None, dlogits=None):
    """The soft-target cross entropy of logits [rows, num_classes] (f32 / bf16, unit column stride) against the NON-binarised mixed
    targets of the batch rows row0 ..: loss (f32 scalar, with workspace = rows f64) and / or dlogits (the logits' dtype) scaled by
    gscale."""
    rows = logits.shape[0] if logits.dim() == 2 else 0
    B = _criterion_args("mix_ce", logits, rows, rows, labels, table, loss, workspace, dlogits)
    t = KERNEL_TIMER.start()
    check(lib().octic_mix_ce(_p(logits), dt_code(logits.dtype), logits.stride(0), _p(labels), _p(table), B, int(row0), rows,
                             logits.shape[1], float(on), float(off), _p(loss), _p(gscale), _p(dlogits),
                             dlogits.stride(0) if dlogits is not None else 0, _p(workspace), _stream(logits)))
    KERNEL_TIMER.stop(t, f"mix_ce_kernel<{_DTN[logits.dtype]}>", logits.numel() * logits.element_size() * (2 if dlogits is not None else 1))


def cosub_bce(logits, labels, table, on, off, binarize, row0=0, loss=None, workspace=None, gscale=None, dlogits=None):
    """The four-term cosub loss of logits [2 rows, num_classes] (first passes, then second passes of the batch rows row0 ..):
    loss (f32 scalar, with workspace = rows f64) and / or dlogits [2 rows, num_classes] scaled by gscale."""
    if logits.dim() != 2 or logits.shape[0] % 2:
        raise ValueError("cosub_bce: logits must be [2 rows, num_classes]: the two passes of every sample")
    rows = logits.shape[0] // 2
    B = _criterion_args("cosub_bce", logits, 2 * rows, rows, labels, table, loss, workspace, dlogits)
    t = KERNEL_TIMER.start()
    check(lib().octic_cosub_bce(_p(logits), dt_code(logits.dtype), logits.stride(0), _p(labels), _p(table), B, int(row0), rows,
                                logits.shape[1], float(on), float(off), int(bool(binarize)), _p(loss), _p(gscale), _p(dlogits),
                                dlogits.stride(0) if dlogits is not None else 0, _p(workspace), _stream(logits)))
    KERNEL_TIMER.stop(t, f"cosub_bce_kernel<{_DTN[logits.dtype]}>", logits.numel() * logits.element_size() * (2 if dlogits is not None else 1))


# ------------------------------------------------------------------------------------------ 3-Augment on uint8 (csrc/augment.hip)
def augment_workspace(B, H, W, device):
    """The int32 workspace octic_augment_u8 needs for a [B, H, W, 3] batch."""
    n = lib().octic_augment_workspace_bytes(int(B), int(H), int(W))
    if n < 0:
        check(int(n))
    return torch.empty(n // 4, dtype=torch.int32, device=device)


def augment_u8(src, table, mean, std, dst, workspace=None):
    """dst = the uint8 batch src [B, H, W, 3] augmented as the device table (AugParams.table()) says; dst is f32 [B, 3, H, W]
    (normalised with mean / std, three floats each) or uint8 [B, H, W, 3] (the pixels in front of ToTensor)."""
    _require_cuda(src)
    _require_cuda(dst)
    _require_cuda(table)
    if src.dim() != 4 or src.shape[3] != 3 or src.dtype != torch.uint8 or not src.is_contiguous():
        raise ValueError("augment_u8: images must be a contiguous uint8 [B, H, W, 3] tensor")
    B, H, W, _ = src.shape
    if table.dtype != torch.int32 or tuple(table.shape) != (B, 16) or not table.is_contiguous():
        raise ValueError(f"augment_u8: the parameter table must be a contiguous int32 [{B}, 16] tensor (AugParams.table())")
    if dst.dtype == torch.float32:
        want, code = (B, 3, H, W), _lib.F32
    elif dst.dtype == torch.uint8:
        want, code = (B, H, W, 3), _lib.U8
    else:
        raise TypeError(f"augment_u8: the output is float32 [B, 3, H, W] or uint8 [B, H, W, 3], got {dst.dtype}")
    if tuple(dst.shape) != want or not dst.is_contiguous():
        raise ValueError(f"augment_u8: the {dst.dtype} output must be a contiguous {want} tensor")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("augment_u8: mean and std take three values each")
    if workspace is None:
        workspace = augment_workspace(B, H, W, src.device)
    elif workspace.dtype != torch.int32 or not workspace.is_cuda or workspace.numel() * 4 < lib().octic_augment_workspace_bytes(B, H, W):
        raise ValueError("augment_u8: the workspace must be an int32 GPU tensor of augment_workspace(B, H, W)'s size")
    t = KERNEL_TIMER.start()
    check(lib().octic_augment_u8(_p(src), _p(dst), code, _p(table), *[float(v) for v in mean], *[float(v) for v in std], B, H, W,
                                 _p(workspace), _stream(src)))
    KERNEL_TIMER.stop(t, "augment_kernel", 2 * src.numel() + dst.numel() * dst.element_size())
    return dst


# ------------------------------------------------------------------------- DINOv2 multi-crop augmentation (csrc/dino_augment.hip)
DINO_ROW_WORDS = 40          # sizeof(octic_dino_row) / 4


def dino_resize_coeffs(n, S, taps):
    """Host: Pillow's 8-bit bicubic coefficients of one axis, crop length n -> S, as numpy (bounds int32 [S, 2], k int32 [S, taps])."""
    import numpy as np
    bounds, k = np.empty((S, 2), np.int32), np.empty((S, taps), np.int32)
    check(lib().octic_dino_resize_coeffs(int(n), int(S), int(taps), bounds.ctypes.data, k.ctypes.data))
    return bounds, k


def dino_resize_max_taps(S):
    """The most taps per output pixel octic_dino_resize_u8 holds at output size S."""
    n = lib().octic_dino_resize_max_taps(int(S))
    if n < 0:
        check(int(n))
    return n


def dino_color_workspace(N, H, W, device):
    """The int32 workspace octic_dino_color_u8 needs for [N, H, W, 3] crops."""
    n = lib().octic_dino_color_workspace_bytes(int(N), int(H), int(W))
    if n < 0:
        check(int(n))
    return torch.empty((n + 3) // 4, dtype=torch.int32, device=device)


def _dino_rows_ok(rows, N, what):
    _require_cuda(rows)
    if rows.dtype != torch.int32 or tuple(rows.shape) != (N, DINO_ROW_WORDS) or not rows.is_contiguous():
        raise ValueError(f"{what}: the rows must be a contiguous int32 [{N}, {DINO_ROW_WORDS}] tensor (DinoAugParams.tables())")


def dino_resize_u8(data, rows, coef, S, crops):
    """crops [N, S, S, 3] (uint8) = the resized, flipped crops the device rows describe, cut from the packed uint8 images
    `data` with the int32 coefficient pool `coef`."""
    for t in (data, coef, crops):
        _require_cuda(t)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("dino_resize_u8: data must be a contiguous 1-D uint8 tensor (PackedImages.data)")
    if coef.dtype != torch.int32 or coef.dim() != 1 or not coef.is_contiguous():
        raise ValueError("dino_resize_u8: the coefficient pool must be a contiguous 1-D int32 tensor")
    N = crops.shape[0]
    if crops.dtype != torch.uint8 or tuple(crops.shape) != (N, S, S, 3) or not crops.is_contiguous():
        raise ValueError(f"dino_resize_u8: the crops must be a contiguous uint8 [N, {S}, {S}, 3] tensor")
    _dino_rows_ok(rows, N, "dino_resize_u8")
    t = KERNEL_TIMER.start()
    check(lib().octic_dino_resize_u8(_p(data), data.numel(), _p(rows), _p(coef), coef.numel(), N, int(S), _p(crops), _stream(data)))
    KERNEL_TIMER.stop(t, "dino_resize_kernel", data.numel() + crops.numel())
    return crops


def dino_color_u8(crops, rows, mean, std, dst, workspace=None):
    """dst = the uint8 crops [N, H, W, 3] through ColorJitter, grayscale, blur and solarize as the device rows say; dst is f32
    [N, 3, H, W] (normalised) or uint8 [N, H, W, 3] (the pixels in front of ToTensor)."""
    _require_cuda(crops)
    _require_cuda(dst)
    if crops.dim() != 4 or crops.shape[3] != 3 or crops.dtype != torch.uint8 or not crops.is_contiguous():
        raise ValueError("dino_color_u8: crops must be a contiguous uint8 [N, H, W, 3] tensor")
    N, H, W, _ = crops.shape
    _dino_rows_ok(rows, N, "dino_color_u8")
    if dst.dtype == torch.float32:
        want, code = (N, 3, H, W), _lib.F32
    elif dst.dtype == torch.uint8:
        want, code = (N, H, W, 3), _lib.U8
    else:
        raise TypeError(f"dino_color_u8: the output is float32 [N, 3, H, W] or uint8 [N, H, W, 3], got {dst.dtype}")
    if tuple(dst.shape) != want or not dst.is_contiguous():
        raise ValueError(f"dino_color_u8: the {dst.dtype} output must be a contiguous {want} tensor")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("dino_color_u8: mean and std take three values each")
    need = lib().octic_dino_color_workspace_bytes(N, H, W)
    if need < 0:
        check(int(need))
    if workspace is None:
        workspace = dino_color_workspace(N, H, W, crops.device)
    elif workspace.dtype != torch.int32 or not workspace.is_cuda or workspace.numel() * 4 < need:
        raise ValueError("dino_color_u8: the workspace must be an int32 GPU tensor of dino_color_workspace(N, H, W)'s size")
    t = KERNEL_TIMER.start()
    check(lib().octic_dino_color_u8(_p(crops), _p(dst), code, _p(rows), *[float(v) for v in mean], *[float(v) for v in std],
                                    N, H, W, _p(workspace), _stream(crops)))
    KERNEL_TIMER.stop(t, "dino_color_kernels", 3 * crops.numel() + dst.numel() * dst.element_size())
    return dst


# ------------------------------------------------------------------------- DeiT crops and evaluation resize (csrc/crop.hip)
CROP_ROW_WORDS = 20          # sizeof(octic_crop_row) / 4


def crop_resize_max_taps(OW):
    """The most taps per output pixel octic_crop_resize_u8 holds for windows OW wide."""
    n = lib().octic_crop_resize_max_taps(int(OW))
    if n < 0:
        check(int(n))
    return n


def crop_resize_rows():
    """Window rows per workgroup of octic_crop_resize_u8."""
    return int(lib().octic_crop_resize_rows())


def crop_resize_u8(data, rows, coef, mean, std, dst):
    """dst = the windows the device rows (octic_crop_row) describe, cut from the packed uint8 images `data` with the int32
    coefficient pool `coef`: uint8 [N, OH, OW, 3], or f32 [N, 3, OH, OW] normalised with mean / std (three floats each)."""
    for t in (data, rows, coef, dst):
        _require_cuda(t)
    if data.dtype != torch.uint8 or data.dim() != 1 or not data.is_contiguous():
        raise ValueError("crop_resize_u8: data must be a contiguous 1-D uint8 tensor (PackedImages.data)")
    if coef.dtype != torch.int32 or coef.dim() != 1 or not coef.is_contiguous():
        raise ValueError("crop_resize_u8: the coefficient pool must be a contiguous 1-D int32 tensor")
    if dst.dim() != 4 or not dst.is_contiguous():
        raise ValueError("crop_resize_u8: the output must be a contiguous uint8 [N, OH, OW, 3] or float32 [N, 3, OH, OW] tensor")
    if dst.dtype == torch.float32 and dst.shape[1] == 3:
        (N, _, OH, OW), code = dst.shape, _lib.F32
    elif dst.dtype == torch.uint8 and dst.shape[3] == 3:
        (N, OH, OW, _), code = dst.shape, _lib.U8
    else:
        raise TypeError(f"crop_resize_u8: the output is float32 [N, 3, OH, OW] or uint8 [N, OH, OW, 3], got {tuple(dst.shape)} {dst.dtype}")
    if rows.dtype != torch.int32 or tuple(rows.shape) != (N, CROP_ROW_WORDS) or not rows.is_contiguous():
        raise ValueError(f"crop_resize_u8: the rows must be a contiguous int32 [{N}, {CROP_ROW_WORDS}] tensor (CropParams.tables())")
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("crop_resize_u8: mean and std take three values each")
    t = KERNEL_TIMER.start()
    check(lib().octic_crop_resize_u8(_p(data), data.numel(), _p(rows), _p(coef), coef.numel(), N, OH, OW, _p(dst), code,
                                     *[float(v) for v in mean], *[float(v) for v in std], _stream(data)))
    KERNEL_TIMER.stop(t, "crop_resize_kernel", data.numel() + dst.numel() * dst.element_size())
    return dst


# ---------------------------------------------------------------------------- linear depth head of the hub (csrc/depth.hip)
DEPTH_BINS = 256


def depth_head_ok(D, layers, n_bins=DEPTH_BINS, upsample=4):
    """The depth kernels take this head (octic_depth_ok, the only place the limits live): D % 64 == 0, 64 <= D <= 4096,
    1 <= layers <= 4, 256 bins, upsample 1 | 2 | 4."""
    return bool(lib().octic_depth_ok(int(D), int(layers), int(n_bins), int(upsample)))


def depth_plan(B, h, w, D, layers, n_bins=DEPTH_BINS, upsample=4):
    """octic_depth_plan: (patch rows per workgroup of the logits launch, its workgroups, chains per logit, workgroups of the
    expectation launch), or None where the launchers refuse the shape."""
    return _lib.plan("octic_depth_plan", int(B), int(h), int(w), int(D), int(layers), int(n_bins), int(upsample))


def _depth_rows(t, what):
    """t ([B, n, D] patch rows or [B, D] class tokens) as the f32 view the kernel reads in place."""
    _require_cuda(t)
    if t.dtype != torch.float32 or t.stride(-1) != 1:
        raise ValueError(f"depth_logits: {what} must be f32 with contiguous channels")
    if t.data_ptr() % 16 or any(s % 4 for s in t.stride()[:-1]):
        raise ValueError(f"depth_logits: {what} needs 16-byte aligned rows (strides that are multiples of 4 floats)")
    return t


def depth_logits(pairs, weight, bias, grid, out=None):
    """Lo [B, h w, 256] f32 = the bin logits of BNHead's 1x1 convolution at patch resolution.  pairs: per layer (patch rows
    [B, h w, D], class token [B, D]) - any views with contiguous channels, read in place (out[:, 1 + R:] and out[:, 0] of a block
    output); weight: f32 [256, 2 D layers] contiguous in the reference's channel order; bias f32 [256]; grid = (h, w)."""
    layers = len(pairs)
    if not 1 <= layers <= 4:
        raise ValueError("depth_logits: 1 to 4 layers")
    h, w = int(grid[0]), int(grid[1])
    B, _, D = pairs[0][0].shape
    dev = pairs[0][0].device
    P, LB, LR, C, CB = _lib.PtrArray4(), _lib.I64Array4(), _lib.I64Array4(), _lib.PtrArray4(), _lib.I64Array4()
    for l, (p, c) in enumerate(pairs):
        if tuple(p.shape) != (B, h * w, D) or tuple(c.shape) != (B, D):
            raise ValueError(f"depth_logits: layer {l} must be ([B, h w, D], [B, D]) = ({(B, h * w, D)}, {(B, D)}), got "
                             f"{tuple(p.shape)}, {tuple(c.shape)}")
        _depth_rows(p, "patch rows")
        _depth_rows(c, "class tokens")
        P[l], LB[l], LR[l], C[l], CB[l] = p.data_ptr(), p.stride(0), p.stride(1), c.data_ptr(), c.stride(0)
    if (weight.dtype != torch.float32 or not weight.is_contiguous() or tuple(weight.shape) != (DEPTH_BINS, 2 * D * layers)
            or bias.dtype != torch.float32 or not bias.is_contiguous() or bias.numel() != DEPTH_BINS
            or weight.device != dev or bias.device != dev):
        raise ValueError(f"depth_logits: weight must be a contiguous f32 [{DEPTH_BINS}, {2 * D * layers}], bias an f32 [{DEPTH_BINS}]")
    if out is None:
        out = torch.empty((B, h * w, DEPTH_BINS), dtype=torch.float32, device=dev)
    elif out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (B, h * w, DEPTH_BINS) or out.device != dev:
        raise ValueError("depth_logits: out must be a contiguous f32 [B, h w, 256] on the operands' device")
    image_bias = torch.empty((B, DEPTH_BINS), dtype=torch.float32, device=dev)
    t = KERNEL_TIMER.start()
    check(lib().octic_depth_logits(P, LB, LR, C, CB, layers, B, h, w, D, _p(weight), _p(bias), DEPTH_BINS, _p(image_bias),
                                   _p(out), _stream(out)))
    KERNEL_TIMER.stop(t, "depth_logits_kernel", 4 * (B * h * w * (D * layers + DEPTH_BINS) + DEPTH_BINS * 2 * D * layers),
                      2.0 * B * h * w * D * layers * DEPTH_BINS)
    return out


def depth_expect(Lo, grid, upsample, bins, min_depth, max_depth, out=None):
    """depth [B, 1, u h, u w] f32 from the patch-level logits Lo [B, h w, 256]: bilinear resize (align_corners=False),
    relu + 0.1, the normalised expectation over bins (f32 [256]) and the clamp to [min_depth, max_depth], one launch."""
    _require_cuda(Lo)
    h, w, u = int(grid[0]), int(grid[1]), int(upsample)
    if Lo.dtype != torch.float32 or not Lo.is_contiguous() or Lo.dim() != 3 or tuple(Lo.shape[1:]) != (h * w, DEPTH_BINS):
        raise ValueError("depth_expect: Lo must be a contiguous f32 [B, h w, 256]")
    if bins.dtype != torch.float32 or not bins.is_contiguous() or bins.numel() != DEPTH_BINS or bins.device != Lo.device:
        raise ValueError("depth_expect: bins must be a contiguous f32 [256] on Lo's device")
    B = Lo.shape[0]
    if out is None:
        out = torch.empty((B, 1, u * h, u * w), dtype=torch.float32, device=Lo.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != B * u * h * u * w or out.device != Lo.device:
        raise ValueError("depth_expect: out must be a contiguous f32 [B, 1, u h, u w] on Lo's device")
    t = KERNEL_TIMER.start()
    check(lib().octic_depth_expect(_p(Lo), B, h, w, DEPTH_BINS, u, _p(bins), float(min_depth), float(max_depth), _p(out),
                                   _stream(Lo)))
    KERNEL_TIMER.stop(t, "depth_expect_kernel", 4 * (Lo.numel() + out.numel()))
    return out


# ------------------------------------------------------------------------------------------ orbit invariants
def _orbit_view(x, c):
    """octic_view of packed rows [..., 8c]: contiguous, or a 2-d row-strided view [M, 8c] (stride(1) == 1)."""
    if x.is_contiguous():
        return pview(x, c)
    _require_cuda(x)
    if x.dim() != 2 or x.shape[1] != 8 * c or x.stride(1) != 1:
        raise ValueError(f"expected packed rows [M, {8 * c}] with unit column stride, got {tuple(x.shape)} / {x.stride()}")
    es, base = x.element_size(), x.data_ptr()
    v = OcticView()
    for i in range(5):
        v.ptr[i] = base + min(i, 4) * c * es
        v.ld[i] = x.stride(0)
    return v


def max_filter_prep(references, dtype):
    """references [R, c, 8] f32 -> the eight component planes [8, R, c] in `dtype` (one launch, nothing cached)."""
    R, c, _ = references.shape
    planes = torch.empty((8, R, c), dtype=dtype, device=references.device)
    check(lib().octic_max_filter_prep(_p(references), _p(planes), R, c, dt_code(dtype), _stream(references)))
    return planes


def max_filter_fwd(x, planes, c, out_dtype):
    """x: packed rows [M, 8c] in the planes' dtype.  Returns (out [M, R] out_dtype, idx [M, R] uint8)."""
    M, R = x.shape[0], planes.shape[1]
    out = torch.empty((M, R), dtype=out_dtype, device=x.device)
    idx = torch.empty((M, R), dtype=torch.uint8, device=x.device)
    xv = _orbit_view(x, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_max_filter_fwd(ctypes.byref(xv), _p(planes), _p(out), _p(idx), M, R, c, dt_code(x.dtype),
                                     dt_code(out_dtype), _stream(x)))
    KERNEL_TIMER.stop(t, "max_filter_fwd_kernel", x.element_size() * 8 * c * (M + R) + M * R * (out.element_size() + 1),
                      24.0 * M * R * c)
    return out, idx


def max_filter_bwd_x(g, idx, planes, c):
    """g [M, R] in the planes' dtype -> dx packed [M, 8c] in that dtype."""
    M, R = g.shape
    dx = torch.empty((M, 8 * c), dtype=planes.dtype, device=g.device)
    dv = pview(dx, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_max_filter_bwd_x(_p(g), _p(idx), _p(planes), ctypes.byref(dv), M, R, c, dt_code(planes.dtype), _stream(g)))
    KERNEL_TIMER.stop(t, "max_filter_bwd_x_kernel", g.element_size() * (M * R + 8 * c * (M + R)) + M * R, 24.0 * M * R * c)
    return dx


def max_filter_bwd_ref_plan(M, R, c):
    """(row slabs, rows per slab, tile edge, workgroups per slab) of max_filter_bwd_ref."""
    answer = _lib.plan("octic_max_filter_bwd_ref_plan", M, R, c)
    if answer is None:
        check(-1)
    return answer


def max_filter_bwd_ref(g, idx, x, c):
    """dref [R, c, 8] f32 from g [M, R] and the packed rows x [M, 8c] (both in the compute dtype)."""
    M, R = g.shape
    need = int(lib().octic_max_filter_bwd_ref_workspace_bytes(M, R, c))
    if need < 0:
        check(need)
    ws = torch.empty(need, dtype=torch.uint8, device=g.device)
    dref = torch.empty((R, c, 8), dtype=torch.float32, device=g.device)
    xv = _orbit_view(x, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_max_filter_bwd_ref(_p(g), _p(idx), ctypes.byref(xv), _p(dref), _p(ws), need, M, R, c, dt_code(g.dtype),
                                         _stream(g)))
    KERNEL_TIMER.stop(t, "max_filter_bwd_ref_kernel", g.element_size() * (M * R + 8 * c * M) + M * R + 2 * need,
                      24.0 * M * R * c)
    return dref


def canonize_fwd(x, reference, c, out_dtype):
    """x packed rows [M, 8c]; reference [8c] f32.  Returns (out [M, 8c] i-major in out_dtype, idx [M] uint8)."""
    M = x.shape[0]
    out = torch.empty((M, 8 * c), dtype=out_dtype, device=x.device)
    idx = torch.empty((M,), dtype=torch.uint8, device=x.device)
    xv = _orbit_view(x, c)
    check(lib().octic_canonize_fwd(ctypes.byref(xv), _p(reference), _p(out), _p(idx), M, c, dt_code(x.dtype), dt_code(out_dtype),
                                   _stream(x)))
    return out, idx


def canonize_bwd(g, idx, c, dtype):
    """g [M, 8c] dense i-major (f32 or bf16) -> dx packed [M, 8c] in `dtype`."""
    M = g.shape[0]
    dx = torch.empty((M, 8 * c), dtype=dtype, device=g.device)
    dv = pview(dx, c)
    check(lib().octic_canonize_bwd(_p(g), dt_code(g.dtype), _p(idx), ctypes.byref(dv), M, c, dt_code(dtype), _stream(g)))
    return dx


# ------------------------------------------------------------------------------------------ polynomial invariants
POLY_MAPS = {"polynomial": (0, 32), "third_order": (1, 15)}       # name -> (OCTIC_POLY_* code, generators)


def _poly_map(map):
    try:
        return POLY_MAPS[map]
    except KeyError:
        raise ValueError(f"poly_invariant: map must be one of {sorted(POLY_MAPS)}, got {map!r}") from None


def poly_invariant_fwd(x, c, map, out_dtype):
    """x: float32 packed rows [..., 8c] (contiguous, or a 2-d row-strided view) -> [..., P c] in out_dtype, generator k of the
    map ("polynomial": P = 32, "third_order": P = 15) at columns [k c, (k + 1) c)."""
    code, P = _poly_map(map)
    if x.dtype != torch.float32:
        raise TypeError(f"poly_invariant_fwd: x must be float32, got {x.dtype}")
    xv = _orbit_view(x, c)
    M = x.numel() // (8 * c)
    out = torch.empty(x.shape[:-1] + (P * c,), dtype=out_dtype, device=x.device)
    t = KERNEL_TIMER.start()
    check(lib().octic_poly_invariant_fwd(ctypes.byref(xv), _p(out), M, c, code, dt_code(out_dtype), _stream(x)))
    KERNEL_TIMER.stop(t, "poly_invariant_fwd_kernel", M * c * (32 + P * out.element_size()))
    return out


def poly_invariant_bwd(g, x, c, map):
    """g: contiguous [..., P c] float32 or bfloat16 cotangent, x as in poly_invariant_fwd -> dx float32, packed like x."""
    code, P = _poly_map(map)
    if x.dtype != torch.float32:
        raise TypeError(f"poly_invariant_bwd: x must be float32, got {x.dtype}")
    M = x.numel() // (8 * c)
    if not g.is_contiguous() or g.numel() != M * P * c or g.device != x.device:
        raise ValueError(f"poly_invariant_bwd: g must be contiguous with {M * P * c} elements on x's device, got {tuple(g.shape)}")
    xv = _orbit_view(x, c)
    dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    dv = pview(dx, c)
    t = KERNEL_TIMER.start()
    check(lib().octic_poly_invariant_bwd(_p(g), dt_code(g.dtype), ctypes.byref(xv), ctypes.byref(dv), M, c, code, _stream(x)))
    KERNEL_TIMER.stop(t, "poly_invariant_bwd_kernel", M * c * (64 + P * g.element_size()))
    return dx
