"""Mixup / CutMix + the BCE loss of the DeiT-III recipe on one MI355X: the kernels of csrc/mixup.hip against the reference's
composition restated with stock torch (timm's Mixup in `batch` mode, `targets.gt(0)`, nn.BCEWithLogitsLoss), at B = 64,
3 x 224 x 224, 1000 classes.

  (a) the data path alone: what lies between a resident batch and the loss gradient, without the model -
      kernels: the table upload, mix_images into the static input buffer, mix_bce forward + backward on resident logits;
      stock:   the in-place mix (`x.mul_(lam).add_(x.flip(0).mul_(1 - lam))` or the box paste), the soft targets, `gt(0)`,
               BCEWithLogitsLoss forward + backward, and the `copy_` of the mixed batch into the static input buffer.
      The arms alternate in one process.  `*_single`: one iteration between two HIP events, the stock arm's work buffer
      refilled from the loader's batch in front of it, untimed (timm mixes in place) - like for like for both arms;
      `kernels_window`: `--window` iterations back to back between one event pair (no idle gaps between launches).  The draws
      are the same seeded sequence for both arms.  Per-kernel times (KERNEL_TIMER, a pass of its own) with achieved GB/s against
      the bytes the algorithm needs.
  (b) `--step MODEL`: the captured training step with the mix inside (`Trainer(mixup=...)`, int64 labels) against the captured
      step fed pre-mixed float targets (`Trainer()` as before this module existed), replays alternating, device time per replay
      with the host running ahead and the host's issue time per replay.

    python tools/bench_mixup.py [--iters 30] [--window 20] [--step hybrid_deit_huge_patch14] [--out profiles/bench_mixup.json]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops  # noqa: E402
from octic_vits_amd.mixup import Mixup, TableUploader, mix_bce_loss, mix_images  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(us):
    return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": len(us)}


def stock_mix(x, y, lam, cut, box, num_classes):
    """timm's `_mix_batch` + `mixup_target` (smoothing 0) + the recipe's `gt(0)`, in place on x."""
    if lam != 1.:
        if cut:
            yl, yh, xl, xh = box
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        else:
            x.mul_(lam).add_(x.flip(0).mul_(1. - lam))
    y1 = torch.zeros(len(y), num_classes, device=y.device).scatter_(1, y.view(-1, 1), 1.0)
    y2 = torch.zeros(len(y), num_classes, device=y.device).scatter_(1, y.flip(0).view(-1, 1), 1.0)
    t = y1 * lam + y2 * (1. - lam)
    return x, t.gt(0.0).type(t.dtype)


def bench_data_path(args, dev):
    B, C, H, W, nc = args.batch, 3, args.img, args.img, args.classes
    g = torch.Generator(device=dev).manual_seed(0)
    fresh = torch.randn(B, C, H, W, generator=g, device=dev)            # the batch as the loader delivers it
    y = torch.randint(0, nc, (B,), generator=g, device=dev)
    logits = torch.randn(B, nc, generator=g, device=dev).to(torch.bfloat16).requires_grad_(True)
    static_in = torch.empty_like(fresh)                                 # the captured step's input buffer
    work = torch.empty_like(fresh)
    crit = torch.nn.BCEWithLogitsLoss()
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=nc, rng=np.random.RandomState(1))
    draws = [mix.draw(B, H, W) for _ in range(args.window)]
    up = TableUploader(B, dev, slots=4)

    def kernel_arm(p):
        table = up.upload(p)
        mix_images(fresh, table, out=static_in)
        logits.grad = None
        mix_bce_loss(logits, y, table, binarize=True).backward()

    def stock_arm(p):
        # timm mixes the loader's batch in place; the loader's copy is not ours to destroy, so the arm starts from `work`, filled
        # outside the timed region (see `timed`)
        x, t = stock_mix(work, y, float(p.lam[0]), bool(p.cut[0]), tuple(int(v) for v in p.box[0]), nc)
        static_in.copy_(x, non_blocking=True)
        logits.grad = None
        crit(logits.float(), t).backward()

    def timed(fn, single):
        """us per iteration over the window's draws.  single: one iteration per event pair, with `work` refilled from the
        loader's batch in front of each, untimed (the stock arm mixes in place); else all of them between one event pair."""
        pair = lambda: (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        if not single:
            e0, e1 = pair()
            e0.record()
            for p in draws:
                fn(p)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / len(draws)
        total = 0.0
        for p in draws:
            work.copy_(fresh)
            e0, e1 = pair()
            e0.record()
            fn(p)
            e1.record()
            torch.cuda.synchronize()
            total += e0.elapsed_time(e1)
        return total * 1e3 / len(draws)

    for _ in range(args.warmup):
        timed(kernel_arm, False)
        timed(stock_arm, True)
    res = {"kernels_window": [], "kernels_single": [], "stock_single": []}
    for _ in range(args.iters):                          # alternating: every arm sees the same machine state
        res["kernels_window"].append(timed(kernel_arm, False))
        res["kernels_single"].append(timed(kernel_arm, True))
        res["stock_single"].append(timed(stock_arm, True))
    out = {"batch": B, "image": [C, H, W], "classes": nc, "window": args.window,
           "what": "us per iteration; *_single = one iteration per event pair (both arms, like for like), kernels_window = "
                   "back-to-back iterations per event pair (no idle gaps)",
           "arms": {k: _stats(v) for k, v in res.items()}}
    out["stock_over_kernels_single"] = round(out["arms"]["stock_single"]["median_us"] / out["arms"]["kernels_single"]["median_us"], 2)
    ops.KERNEL_TIMER.enable()
    for p in draws:
        kernel_arm(p)
    out["kernels"] = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    # mix_images: the sample and its partner read, the result written (the partner mostly from L2: counted, so a lower bound on GB/s)
    out["mix_images_alg_MB"] = round(12 * fresh.numel() / 1e6, 1)
    return out


def bench_step(args, dev):
    from octic_vits_amd.deit_models import create_model
    from octic_vits_amd.train import Trainer
    nc, B = args.classes, args.batch
    g = torch.Generator(device=dev).manual_seed(2)
    batches = [(torch.randn(B, 3, args.img, args.img, generator=g, device=dev), torch.randint(0, nc, (B,), generator=g, device=dev))
               for _ in range(3)]
    mix_kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=nc)
    pre = Mixup(rng=np.random.RandomState(3), **mix_kw)
    premixed = [pre.apply(x, y, binarize=True) for x, y in batches]
    arms = {}
    for name in ("mixup_inside", "premixed_targets"):
        torch.manual_seed(0)
        model = create_model(args.step, num_classes=nc, drop_path_rate=0.5, img_size=args.img).to(dev)
        if name == "mixup_inside":
            tr = Trainer(model, mixup=Mixup(rng=np.random.RandomState(3), **mix_kw))
            arms[name] = (tr.capture(*batches[0]), batches)
        else:
            tr = Trainer(model)
            arms[name] = (tr.capture(*premixed[0]), premixed)
    for gs, data in arms.values():
        for x, y in data:
            gs.replay(x, y)
    torch.cuda.synchronize()
    out = {"model": args.step, "batch": B, "replays_per_window": args.step_window}
    samples = {k: [] for k in arms}
    host = {k: [] for k in arms}
    for _ in range(args.step_iters):                     # alternating windows of replays, the host running ahead inside a window
        for k, (gs, data) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(args.step_window):
                t0 = time.perf_counter()
                gs.replay(*data[i % len(data)])
                host[k].append((time.perf_counter() - t0) * 1e3)
            e1.record()
            torch.cuda.synchronize()
            samples[k].append(e0.elapsed_time(e1) / args.step_window)
    for k in arms:
        ms = sorted(samples[k])
        out[k] = {"ms_per_replay": {"median": round(_median(ms), 3), "min": round(ms[0], 3), "max": round(ms[-1], 3), "n": len(ms)},
                  "host_issue_ms": round(_median(host[k]), 3), "images_per_s": round(B / _median(ms) * 1e3, 1)}
    out["mixup_inside_minus_premixed_ms"] = round(out["mixup_inside"]["ms_per_replay"]["median"]
                                                  - out["premixed_targets"]["ms_per_replay"]["median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--img", type=int, default=224)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--step", default=None, metavar="MODEL", help="also time the captured training step of this deit_models name")
    ap.add_argument("--step-iters", type=int, default=6)
    ap.add_argument("--step-window", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixup: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "data_path": bench_data_path(args, dev)}
    if args.step:
        res["captured_step"] = bench_step(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
