"""One ``TopkAccuracy.update`` at the linear probe's shape on one MI355X: 48 classifiers x 1024 images x 1000 classes of f32
logits resident on the device, top-1 and top-5.

Variants: the plain metric (mean accuracy), the 200-class mapping of ImageNet-A / -R, per-class counters, ImageNet-ReaL with 10
targets per row (half of them -1).
Arms, alternating in one process on the same tensors:
  kernels  ``metrics.TopkAccuracy.update``: ``octic_topk_rank`` + ``octic_topk_count`` (2 launches for all classifiers);
  torch    the reference's composition (dinov2/eval/metrics.py on torchmetrics' ``select_topk``) on stock torch, batched over the
           48 classifiers, which is kinder than the reference's loop over classifiers and over k: the column gather
           ``preds[..., class_mapping]`` under a mapping, ``topk(k)`` and the one-hot ``scatter_`` per k, then the gather at the
           target and a sum (mean accuracy), an ``index_add_`` / ``bincount`` per class (per-class), or the product with the
           one-hot of the padded targets, its clipped row sum and the mask (ReaL).
Both arms leave their counts on the device (no read-back inside the timed window).  Timing: `--window` updates between one pair
of HIP events after a warm-up of every variant; the median over `--iters` windows with minimum and maximum, in microseconds per
update.  Bytes moved by the kernels' arm are counted from the shapes (the scores once, the mapping, targets, ranks and counters)
and given as a rate and as a fraction of the 8.0 TB/s HBM3E peak (6.3 TB/s is what a float4 copy reaches).  The counts of the two
arms are compared on rows of pairwise distinct scores, where ``topk`` is determined.

    python tools/bench_metrics.py [--iters 20] [--window 50] [--out profiles/bench_metrics.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import metrics  # noqa: E402

HBM_PEAK = 8.0e12
KS = (1, 5)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def window_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def onehot_topk(preds, k):
    return torch.zeros_like(preds, dtype=torch.int32).scatter_(-1, preds.topk(k, dim=-1).indices, 1)


class TorchArm:
    """The stock-torch composition with device accumulators laid out as TopkAccuracy.counters."""

    def __init__(self, variant, G, Cm, mapping):
        self.variant, self.G, self.Cm = variant, G, Cm
        self.mapping = None if mapping is None else torch.as_tensor(mapping, device="cuda").long()
        shape = (G, Cm, 1 + len(KS)) if variant == "per_class" else (G, 1 + len(KS))
        self.counters = torch.zeros(shape, dtype=torch.int64, device="cuda")

    def update(self, scores, targets):
        preds = scores if self.mapping is None else scores[..., self.mapping]
        G, n, Cm = preds.shape
        if self.variant == "real":
            t = torch.where(targets < 0, torch.full_like(targets, Cm), targets)
            target_oh = torch.zeros(n, Cm + 1, dtype=torch.int32, device=preds.device).scatter_(1, t, 1)[:, :Cm]
            defined = target_oh.sum(1) > 0
            self.counters[:, 0] += defined.sum()
            for i, k in enumerate(KS):
                tp = (onehot_topk(preds, k) * target_oh).sum(-1).clip_(max=1)
                self.counters[:, 1 + i] += (tp * defined).sum(-1)
            return
        idx = targets.view(1, n, 1).expand(G, n, 1)
        if self.variant == "per_class":
            self.counters[:, :, 0] += torch.bincount(targets, minlength=Cm)
        else:
            self.counters[:, 0] += n
        for i, k in enumerate(KS):
            hit = onehot_topk(preds, k).gather(-1, idx)[..., 0].long()
            if self.variant == "per_class":
                self.counters[:, :, 1 + i].index_add_(1, targets, hit)
            else:
                self.counters[:, 1 + i] += hit.sum(-1)


def bench(variant, G, n, C, args, lines):
    g = torch.Generator().manual_seed(len(variant))
    # pairwise distinct scores per row: both arms must count the same
    scores = (torch.argsort(torch.rand(G, n, C, generator=g), dim=-1).float() * 0.01 - 5.0).to("cuda")
    mapping = torch.randperm(C, generator=g)[:200].tolist() if variant == "mapped" else None
    Cm = C if mapping is None else len(mapping)
    A = 10 if variant == "real" else 1
    targets = torch.randint(0, Cm, (n, A), generator=g)
    if variant == "real":
        targets[torch.rand(n, A, generator=g) < 0.5] = -1
    targets = (targets if A > 1 else targets.view(n)).to("cuda")
    mt = {"plain": "mean_accuracy", "mapped": "mean_accuracy", "per_class": "per_class_accuracy", "real": "imagenet_real_accuracy"}[variant]
    ours = metrics.TopkAccuracy(mt, Cm, ks=KS, groups=G, class_mapping=mapping, tie="strict", device="cuda")
    theirs = TorchArm(variant, G, Cm, mapping)
    arms = {"kernels": lambda: ours.update(scores, targets), "torch": lambda: theirs.update(scores, targets)}
    for fn in arms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    same = torch.equal(ours.counters, theirs.counters)
    res = {name: [] for name in arms}
    for _ in range(args.iters):
        for name, fn in arms.items():
            res[name].append(window_us(fn, args.window))
    k, t = _median(res["kernels"]), _median(res["torch"])
    nbytes = G * n * Cm * 4 + (4 * Cm if mapping is not None else 0) + 8 * n * A + 2 * 4 * G * n * A + 8 * ours.counters.numel()
    rate = nbytes / (k * 1e-6)
    lines.append(f"  {variant:9s} G {G} n {n} C {C} Cm {Cm} A {A:2d}   kernels {k:8.1f} ({min(res['kernels']):.1f}, {max(res['kernels']):.1f}) us"
                 f"   torch {t:9.1f} ({min(res['torch']):.1f}, {max(res['torch']):.1f}) us   torch / kernels {t / k:6.2f}"
                 f"   kernels' arm moves {nbytes / 1e6:.1f} MB: {rate / 1e12:.2f} TB/s = {100.0 * rate / HBM_PEAK:.0f}% of HBM peak"
                 f"   counters {'equal' if same else 'DIFFER'}")
    return same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=50)
    ap.add_argument("--groups", type=int, default=48)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics: needs a GPU (no CPU path)")
    lines = [f"bench_metrics: {torch.cuda.get_device_name(0)}, one update of top-1 / top-5 counters on resident f32 scores, us per update: "
             f"median (min, max) of {args.iters} windows of {args.window} updates, arms alternating"]
    ok = True
    for variant in ("plain", "mapped", "per_class", "real"):
        ok = bench(variant, args.groups, args.rows, args.classes, args, lines) and ok
        print(lines[-1], flush=True)
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit("bench_metrics: the two arms counted differently")


if __name__ == "__main__":
    main()
