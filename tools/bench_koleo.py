"""The KoLeo regularizer of the DINOv2 step on one MI355X: forward + backward of ``ssl.KoLeoLoss.forward_groups(x, 2)`` summed over
the two global crops, as `SSLMetaArch.forward_backward` runs it, on resident class tokens x [2 n, D].

Arms, alternating in one process on the same seeded x:
  kernels  csrc/koleo.hip: one forward and one backward launch for both crops (+ the mean and the sum in torch);
  eager    ``FUSED_LOSS_ROWS = False``: the composition the step ran before, per crop: cast, F.normalize, an n x n torch.mm on the
           BLAS library, the diagonal fill, max, the gather, PairwiseDistance, log, mean and the autograd backward of each.
Each arm is captured once as a hipGraph and replayed `--window` times between one pair of HIP events (device time with the launches'
host cost removed: what the term costs inside a captured step, and the kinder setting for the eager arm, whose ~100 launches are
host-bound outside a graph).  Reported: the median over `--iters` windows, with minimum and maximum, in microseconds per iteration,
the ratio eager / kernels, and the kernel launches of one iteration of each arm (counted by the profiler outside the timed windows).

    python tools/bench_koleo.py [--iters 20] [--window 100] [--out profiles/bench_koleo.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ssl as S  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def make_arm(x, fused):
    kl = S.KoLeoLoss()

    def it():
        S.FUSED_LOSS_ROWS = fused
        try:
            x.grad = None
            loss = sum(kl.forward_groups(x, 2).unbind(0))
            loss.backward()
            return loss
        finally:
            S.FUSED_LOSS_ROWS = True
    return it


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def count_launches(fn):
    """Kernel launches of one iteration (None where the profiler is not available)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
                and not e.name.lower().startswith(("memcpy", "memset")))
        return n or None
    except Exception:
        return None


def bench(n, D, dtype, args, lines, count):
    g = torch.Generator(device="cuda").manual_seed(n + D)
    x = torch.randn(2 * n, D, generator=g, device="cuda").to(dtype).requires_grad_(True)
    arms = {"kernels": make_arm(x, True), "eager": make_arm(x, False)}
    losses, grads, graphs = {}, {}, {}
    for name, it in arms.items():                        # warm-up; parity of value and gradient while we are here
        for _ in range(3):
            losses[name] = float(it().detach())
        grads[name] = x.grad.detach().float().clone()
    launches = {name: (count_launches(it) if count else None) for name, it in arms.items()}
    for name, it in arms.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            it()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        x.grad = None
        with torch.cuda.graph(graph):
            it()
        graphs[name] = graph.replay
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    res = {name: [] for name in arms}
    for _ in range(args.iters):                          # alternating: every arm sees the same machine state
        for name in arms:
            res[name].append(window_us(graphs[name], args.window))
    k, e = _median(res["kernels"]), _median(res["eager"])
    gmax = float(grads["eager"].abs().max())
    ln = lambda v: "not counted" if v is None else f"{v} launches"
    lines.append(f"  {str(dtype)[6:]:8s} n {n:3d} D {D:4d}   kernels {k:7.1f} ({min(res['kernels']):.1f}, {max(res['kernels']):.1f}) [{ln(launches['kernels'])}]"
                 f"   eager {e:7.1f} ({min(res['eager']):.1f}, {max(res['eager']):.1f}) [{ln(launches['eager'])}]   eager / kernels {e / k:5.2f}"
                 f"   loss {losses['kernels']:.6f} / {losses['eager']:.6f}  max |dx diff| / max |dx| {float((grads['kernels'] - grads['eager']).abs().max()) / gmax:.1e}")
    return e / k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--n", type=int, nargs="+", default=[16, 32, 64, 128, 256])
    ap.add_argument("--dims", type=int, nargs="+", default=[1024, 1280, 1536])
    ap.add_argument("--no-count", action="store_true", help="skip the profiler's launch count")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_koleo: needs a GPU (no CPU path)")
    lines = [f"bench_koleo: {torch.cuda.get_device_name(0)}, G = 2 crops, forward + backward of the KoLeo term inside a hipGraph, us per "
             f"iteration: median (min, max) of {args.iters} windows of {args.window} replays, arms alternating"]
    worst = None
    for dtype in (torch.bfloat16, torch.float32):
        for n in args.n:
            for D in args.dims:
                r = bench(n, D, dtype, args, lines, count=not args.no_count and D == args.dims[0])
                worst = r if worst is None else min(worst, r)
                print(lines[-1], flush=True)
    lines.append(f"  smallest eager / kernels over all shapes: {worst:.2f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
