"""Developer micro-benchmark: the float32 attention kernels (csrc/attn_f32.hip, octic_attn_{fwd,bwd}_f32) against the path
they replace, F.scaled_dot_product_attention on the same float32 [B,H,T,hd] tensors - forward and forward + backward.

Both sides run in one process, alternating round by round with the order inside a round swapped every round (HIP, SDPA,
SDPA, HIP, HIP, SDPA, ...), each round a device-event window of `--iters` calls after a warm-up of every shape; the
table shows the median round of each side, the spread (min .. max), the ratio of medians (HIP / SDPA: <= 1.0 means the kernels are not slower) and the achieved share of the
157 TF f32 MFMA peak (4 T^2 hd FLOP per head forward, 14 T^2 hd backward: dq 3 products, dk / dv 4; the SDPA rows are
counted with the same FLOPs so that the columns compare times).

    python tools/bench_attn_f32.py                      # the three shapes of the NOTES table
    python tools/bench_attn_f32.py --rounds 10 --iters 10
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from octic_vits_amd import functional as OF

PEAK_F32_MFMA = 157e12
SHAPES = [(64, 16, 257, 80), (64, 16, 197, 64), (8, 16, 1370, 80)]


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, rounds, iters):
    """fns: {label: callable} -> {label: [ms per round]}, the sides taking turns inside every round"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {label: [] for label in fns}
    order = list(fns.items())
    for r in range(rounds):
        for label, fn in (order if r % 2 == 0 else order[::-1]):     # who goes first swaps every round
            out[label].append(window(fn, iters))
    return out


def line(label, ms, flops):
    med = statistics.median(ms)
    return (f"  {label:<22s} median {med:8.3f} ms  (min {min(ms):8.3f}, max {max(ms):8.3f})  {flops / med / 1e9:7.1f} TF/s  "
            f"{100 * flops / (med * 1e-3) / PEAK_F32_MFMA:5.1f} % of the f32 MFMA peak")


def bench(B, H, T, hd, rounds, iters):
    sc = hd ** -0.5
    q, k, v = (torch.randn(B, H, T, hd, device="cuda").requires_grad_(True) for _ in range(3))
    do = torch.randn(B, H, T, hd, device="cuda")
    ff, fb = 4.0 * B * H * T * T * hd, 14.0 * B * H * T * T * hd

    def hip(backward):
        out = OF.AttnFn.apply(q, k, v, sc)
        if backward:
            torch.autograd.grad(out, (q, k, v), do)

    def sdpa(backward):
        out = F.scaled_dot_product_attention(q, k, v)
        if backward:
            torch.autograd.grad(out, (q, k, v), do)

    with torch.no_grad():
        fwd = alternate({"HIP": lambda: hip(False), "SDPA": lambda: sdpa(False)}, rounds, iters)
    both = alternate({"HIP": lambda: hip(True), "SDPA": lambda: sdpa(True)}, rounds, iters)
    o_h = OF.AttnFn.apply(q, k, v, sc)
    o_s = F.scaled_dot_product_attention(q, k, v)
    print(f"float32 [B,H,T,hd] = ({B},{H},{T},{hd})   max |HIP - SDPA| = {(o_h - o_s).abs().max().item():.2e}")
    print(line("HIP fwd", fwd["HIP"], ff))
    print(line("SDPA fwd", fwd["SDPA"], ff))
    print(line("HIP fwd + bwd", both["HIP"], ff + fb))
    print(line("SDPA fwd + bwd", both["SDPA"], ff + fb))
    rf = statistics.median(fwd["HIP"]) / statistics.median(fwd["SDPA"])
    rb = statistics.median(both["HIP"]) / statistics.median(both["SDPA"])
    print(f"  ratio of medians HIP / SDPA: fwd {rf:.3f}, fwd + bwd {rb:.3f}")
    return rf, rb


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_f32: needs a GPU")
    torch.manual_seed(0)
    print(f"SDPA backends enabled: flash {torch.backends.cuda.flash_sdp_enabled()}, "
          f"mem-efficient {torch.backends.cuda.mem_efficient_sdp_enabled()}, math {torch.backends.cuda.math_sdp_enabled()}")
    for shape in SHAPES:
        bench(*shape, args.rounds, args.iters)
