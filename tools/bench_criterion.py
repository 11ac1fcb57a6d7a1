"""The fused criteria of csrc/mixup.hip on one MI355X: forward + backward of `mixup.mix_ce_loss` (soft-target cross entropy) and
`mixup.cosub_bce_loss` (the four BCE terms of --cosub) on resident bf16 logits against the reference loop's composition restated
with stock torch on materialised targets, at rows = 64 and C = 1000 (ImageNet-1k) and 21841 (ImageNet-21k).

Arms, alternating in one process, the same seeded table, labels and logits for all:
  kernels        the fused loss and its backward: 2 + 1 launches (row kernel + finish, row kernel), no [rows, C] targets;
  stock          `sum(-t * log_softmax(x.float()), -1).mean()` (timm's SoftTargetCrossEntropy) / the four
                 `F.binary_cross_entropy_with_logits` terms of deit/engine.py:61-65, on targets that are already there;
  stock+targets  the same behind `mixup.mix_targets` (the targets have to come from somewhere every step).
Each arm is timed twice: `eager` - `--window` iterations back to back between one pair of HIP events (what a step outside a graph
pays: the larger of the host's issue time and the device's), and `graph` - the same iteration captured once as a hipGraph and
replayed `--window` times between one event pair (what it costs inside `Trainer.capture`: device time with the launches' host
cost removed).  Reported: the median over `--iters` windows, with minimum and maximum, in microseconds per iteration.

    python tools/bench_criterion.py [--iters 20] [--window 50] [--out profiles/bench_criterion.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd.mixup import Mixup, cosub_bce_loss, mix_ce_loss, mix_targets  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def soft_target_ce(x, t):
    return torch.sum(-t * F.log_softmax(x.float(), dim=-1), dim=-1).mean()


def cosub_stock(x, t):
    bce = F.binary_cross_entropy_with_logits
    a, b = torch.split(x.float(), x.shape[0] // 2, dim=0)
    loss = 0.25 * bce(a, t)
    loss = loss + 0.25 * bce(b, t)
    loss = loss + 0.25 * bce(a, b.detach().sigmoid())
    return loss + 0.25 * bce(b, a.detach().sigmoid())


def make_arms(kind, rows, C, dev):
    g = torch.Generator(device=dev).manual_seed(rows + C)
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=C, mode="elem", rng=np.random.RandomState(1))
    table = torch.from_numpy(mix.draw(rows, 224, 224).table()).to(dev)
    y = torch.randint(0, C, (rows,), generator=g, device=dev)
    on, off = mix.on_off()
    n = rows if kind == "ce" else 2 * rows
    logits = (3 * torch.randn(n, C, generator=g, device=dev)).to(torch.bfloat16).requires_grad_(True)
    binarize = False
    ready = mix_targets(y, table, C, on=on, off=off, binarize=binarize)
    if kind == "ce":
        fused = lambda: mix_ce_loss(logits, y, table, on=on, off=off)
        stock = lambda t: soft_target_ce(logits, t)
    else:
        fused = lambda: cosub_bce_loss(logits, y, table, on, off, binarize)
        stock = lambda t: cosub_stock(logits, t)

    def run(loss_fn):
        def it():
            logits.grad = None
            loss = loss_fn()
            loss.backward()
            return loss
        return it

    arms = {"kernels": run(fused), "stock": run(lambda: stock(ready)),
            "stock+targets": run(lambda: stock(mix_targets(y, table, C, on=on, off=off, binarize=binarize)))}
    return arms, logits


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def bench(kind, rows, C, args, dev, lines):
    arms, logits = make_arms(kind, rows, C, dev)
    losses, grads = {}, {}
    for name, it in arms.items():                        # warm-up; parity of value and gradient while we are here
        for _ in range(3):
            losses[name] = float(it().detach())
        grads[name] = logits.grad.detach().float().clone()
    graphs = {}
    for name, it in arms.items():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            it()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        logits.grad = None
        with torch.cuda.graph(graph):
            it()
        graphs[name] = graph.replay
        for _ in range(3):
            graph.replay()
    torch.cuda.synchronize()
    res = {(mode, name): [] for mode in ("eager", "graph") for name in arms}
    for _ in range(args.iters):                          # alternating: every arm sees the same machine state
        for name in arms:
            res[("eager", name)].append(window_us(arms[name], args.window))
            res[("graph", name)].append(window_us(graphs[name], args.window))
    what = "mix_ce_loss" if kind == "ce" else "cosub_bce_loss"
    shape = f"{rows} x {C}" if kind == "ce" else f"2 x {rows} x {C}"
    mb = logits.numel() * 2 / 1e6
    lines.append(f"{what}  bf16 logits {shape} ({mb:.2f} MB), forward + backward, us per iteration: median (min, max) of {args.iters} "
                 f"windows of {args.window}")
    for mode in ("eager", "graph"):
        base = _median(res[(mode, "kernels")])
        for name in arms:
            v = res[(mode, name)]
            rel = "" if name == "kernels" else f"   {_median(v) / base:5.2f} x the kernels"
            lines.append(f"    {mode:5s}  {name:14s} {_median(v):8.1f}  ({min(v):.1f}, {max(v):.1f}){rel}")
    gmax = float(grads["stock"].abs().max())
    lines.append(f"    parity   loss: kernels {losses['kernels']:.7g}  stock {losses['stock']:.7g};  max |dlogits difference| / max |dlogits| "
                 f"= {float((grads['kernels'] - grads['stock']).abs().max()) / gmax:.2e} (bf16 gradients)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--classes", type=int, nargs="+", default=[1000, 21841])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_criterion: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    lines = [f"bench_criterion: {torch.cuda.get_device_name(0)}, rows {args.rows}, smoothing 0.1, elem-mode Mixup / CutMix table"]
    for kind in ("ce", "cosub"):
        for C in args.classes:
            bench(kind, args.rows, C, args, dev, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
