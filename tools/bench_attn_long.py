"""Developer micro-benchmark: the long-sequence attention kernels (csrc/attn_stream.hip) against the paths they replace -
pack -> F.scaled_dot_product_attention -> unpack (AttentionD8 above 320 tokens before) and plain SDPA on [B,H,T,hd] (the
standard blocks) - forward and forward + backward, in ms and TF/s (4 T^2 hd per head forward, 14 T^2 hd backward for the
HIP pair; the SDPA rows are counted with the same FLOPs so that the columns compare times).

    python tools/bench_attn_long.py            # the three shapes of the NOTES table
    python tools/bench_attn_long.py --knob     # also the streaming kernels at T = 197 / 257 (OCTIC_ROUTE_ATTN_STREAM = 1)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from octic_vits_amd import _lib, functional as OF, ops


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def row(label, ms, flops):
    return f"  {label:<34s} {ms:8.3f} ms {flops / ms / 1e9:8.1f} TF/s"


def packed(B, H, T, w):
    c, hd = w * H, 8 * w
    sc = hd ** -0.5
    qkv = (torch.randn(B, T, 24 * c, device="cuda") * 0.7).bfloat16()
    do = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    ff, fb = 4.0 * B * H * T * T * hd, 14.0 * B * H * T * T * hd
    o, lse = ops.attn_fwd_packed(qkv, H, c, sc)
    hf = timeit(lambda: ops.attn_fwd_packed(qkv, H, c, sc))
    hb = timeit(lambda: ops.attn_bwd_packed(qkv, o, do, lse, H, c, sc))
    q = qkv.detach().requires_grad_(True)

    def sdpa(backward):
        a, b, v = OF.PackHeadsFn.apply(q, H, c)
        out = OF.UnpackHeadsFn.apply(F.scaled_dot_product_attention(a, b, v), c)
        if backward:
            torch.autograd.grad(out, q, do)
    with torch.no_grad():
        sf = timeit(lambda: sdpa(False))
    sfb = timeit(lambda: sdpa(True))
    print(f"packed rows B {B} H {H} T {T} hd {hd}")
    print(row("HIP fwd (attn_fwd_stream_kernel)", hf, ff))
    print(row("HIP bwd (dq + dkv stream kernels)", hb, fb))
    print(row("HIP fwd + bwd", hf + hb, ff + fb))
    print(row("pack -> SDPA -> unpack fwd", sf, ff))
    print(row("pack -> SDPA -> unpack fwd + bwd", sfb, ff + fb))


def strided(B, H, T, hd):
    sc = hd ** -0.5
    qkv = torch.randn(B, T, 3, H, hd, device="cuda").bfloat16()
    do = torch.randn(B, T, H * hd, device="cuda").bfloat16()
    ff, fb = 4.0 * B * H * T * T * hd, 14.0 * B * H * T * T * hd
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    hf = timeit(lambda: ops.attn_fwd(q, k, v, sc))
    x = qkv.detach().requires_grad_(True)

    def hip():
        out = OF.AttnFusedQKVFn.apply(x, sc)
        torch.autograd.grad(out, x, do)

    def sdpa(backward):
        a, b, v = x.permute(2, 0, 3, 1, 4).unbind(0)
        out = F.scaled_dot_product_attention(a, b, v).transpose(1, 2).reshape(B, T, H * hd)
        if backward:
            torch.autograd.grad(out, x, do)
    hfb = timeit(hip)
    with torch.no_grad():
        sf = timeit(lambda: sdpa(False))
    sfb = timeit(lambda: sdpa(True))
    print(f"strided [B,T,3,H,hd] views B {B} H {H} T {T} hd {hd}")
    print(row("HIP fwd (attn_fwd_stream_kernel)", hf, ff))
    print(row("HIP fwd + bwd", hfb, ff + fb))
    print(row("SDPA fwd", sf, ff))
    print(row("SDPA fwd + bwd", sfb, ff + fb))


def knob(B, H, T, w):
    c, hd = w * H, 8 * w
    sc = hd ** -0.5
    qkv = (torch.randn(B, T, 24 * c, device="cuda") * 0.7).bfloat16()
    do = torch.randn(B, T, 8 * c, device="cuda").bfloat16()
    ff, fb = 4.0 * B * H * T * T * hd, 14.0 * B * H * T * T * hd
    for v in (0, 1):
        _lib.route_override(_lib.ROUTE_ATTN_STREAM, v)
        o, lse = ops.attn_fwd_packed(qkv, H, c, sc)
        hf = timeit(lambda: ops.attn_fwd_packed(qkv, H, c, sc))
        hb = timeit(lambda: ops.attn_bwd_packed(qkv, o, do, lse, H, c, sc))
        print(f"packed rows B {B} H {H} T {T} hd {hd}, ROUTE_ATTN_STREAM = {v}")
        print(row("fwd", hf, ff))
        print(row("bwd", hb, fb))
    _lib.route_override(_lib.ROUTE_ATTN_STREAM, 0)


if __name__ == "__main__":
    torch.manual_seed(0)
    print(f"SDPA backends enabled: flash {torch.backends.cuda.flash_sdp_enabled()}, "
          f"mem-efficient {torch.backends.cuda.mem_efficient_sdp_enabled()}, math {torch.backends.cuda.math_sdp_enabled()}")
    packed(16, 16, 1025, 10)
    packed(32, 16, 577, 8)
    strided(4, 16, 2049, 80)
    if "--knob" in sys.argv:
        knob(64, 16, 257, 10)
        knob(64, 16, 197, 8)
