"""Linear-probe iteration on one MI355X: the engine's four launches against the reference's composition restated with stock
torch (dinov2/eval/linear.py:344-366: one nn.Linear + CrossEntropyLoss per classifier, torch.optim.SGD(momentum=0.9)).

  (a) the probe alone on resident feature rows (B = 128, D = 1280, C = 1000, the 52-classifier grid): engine vs stock with
      the default and the foreach=True optimizer, arms interleaved in one process, HIP events around each iteration; per-kernel
      times (KERNEL_TIMER, a pass of its own) with achieved GB/s and TFLOP/s against the bytes and flops the algorithm needs;
  (b) the whole iteration with the hybrid ViT-H/16 backbone at 224 x 224 under bf16 autocast: eager vs captured, with the
      host's issue time per iteration.

    python tools/bench_probe.py [--iters 50] [--warmup 5] [--skip-backbone] [--out profiles/bench_probe.json]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octic_vits_amd import ops, probe  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(ms):
    return {"median_ms": round(_median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}


class StockProbe:
    """The reference's classifiers and optimizer as stock torch modules on the same feature rows."""

    def __init__(self, p, foreach):
        self.slices = [(h["col0"], h["col0"] + h["out_dim"]) for h in p.heads.values()]
        self.mods = [torch.nn.Linear(h["out_dim"], p.num_classes).to(p.device) for h in p.heads.values()]
        with torch.no_grad():
            for m, n in zip(self.mods, p.names):
                m.weight.copy_(p.weights[n])
                m.bias.copy_(p.biases[n])
        groups = [{"params": list(m.parameters()), "lr": h["lr"]} for m, h in zip(self.mods, p.heads.values())]
        self.opt = torch.optim.SGD(groups, momentum=0.9, weight_decay=0, foreach=foreach)
        self.crit = torch.nn.CrossEntropyLoss()

    def step(self, F, labels):
        # create_linear_input builds each classifier's input with torch.cat: a column range of F, made contiguous, costs the same copy
        losses = [self.crit(m(F[:, a:b].contiguous()), labels) for m, (a, b) in zip(self.mods, self.slices)]
        loss = sum(losses)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        return loss


def timed(fn, sync=True):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    host = (time.perf_counter() - t0) * 1e3
    if sync:
        torch.cuda.synchronize()
    return e0, e1, host


def bench_probe_alone(args, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    p = probe.LinearProbe(None, embed_dim=args.dim, num_classes=args.classes, batch_size=args.batch, world_size=args.world,
                          device=dev, generator=g)
    opt = probe.ProbeSGD(p)
    F = torch.randn(args.batch, p.width, generator=g, device=dev)
    labels = torch.randint(0, args.classes, (args.batch,), generator=g, device=dev)
    arms = {"engine": lambda: p.step_features(F, labels)}
    for name, foreach in (("stock_sgd_default", None), ("stock_sgd_foreach", True)):
        s = StockProbe(p, foreach)
        arms[name] = (lambda s=s: s.step(F, labels))
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = {k: [] for k in arms}, {k: [] for k in arms}
    for _ in range(args.iters):                               # interleaved: every arm sees the same machine state
        for k, fn in arms.items():
            e0, e1, host = timed(fn)
            dev_ms[k].append(e0.elapsed_time(e1))
            host_ms[k].append(host)
    out = {"classifiers": len(p), "batch": args.batch, "dim": args.dim, "classes": args.classes,
           "weights_M": round(args.classes * p.sum_k / 1e6, 2),
           "arms": {k: {"device": _stats(dev_ms[k]), "host_issue": _stats(host_ms[k])} for k in arms}}
    eng = out["arms"]["engine"]["device"]["median_ms"]
    for k in arms:
        out["arms"][k]["vs_engine"] = round(out["arms"][k]["device"]["median_ms"] / eng, 2)
    # algorithmic traffic and work of one engine iteration: W read by the forward (4 B), W + momentum read and written by the
    # update (16 B); two GEMMs of 2 B C sum(K) flops
    nbytes = 20.0 * args.classes * p.sum_k
    flops = 4.0 * args.batch * args.classes * p.sum_k
    out["engine_total"] = {"alg_GB": round(nbytes / 1e9, 3), "alg_GFLOP": round(flops / 1e9, 1),
                           "GBps": round(nbytes / eng / 1e6, 1), "TFLOPs": round(flops / eng / 1e9, 1)}
    ops.KERNEL_TIMER.enable()
    for _ in range(max(5, args.iters // 5)):
        p.step_features(F, labels)
    out["engine_kernels"] = ops.KERNEL_TIMER.summary()
    ops.KERNEL_TIMER.disable()
    return out


def bench_with_backbone(args, dev):
    from octic_vits_amd import dinov2_models
    torch.manual_seed(0)
    model = dinov2_models.hybrid_dinov2_vit_huge_patch16().to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(args.batch, 3, 224, 224, generator=g, device=dev)
    y = torch.randint(0, args.classes, (args.batch,), generator=g, device=dev)
    out = {}
    pe = probe.LinearProbe(model, num_classes=args.classes, batch_size=args.batch, world_size=args.world, generator=g)
    probe.ProbeSGD(pe)
    pc = probe.LinearProbe(model, num_classes=args.classes, batch_size=args.batch, world_size=args.world, generator=g)
    probe.ProbeSGD(pc)
    replay = pc.capture(x, y)
    arms = {"eager": lambda: pe.step(x, y), "captured": lambda: replay(x, y)}
    for _ in range(args.warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    n = max(10, args.iters // 2)
    for k, fn in arms.items():
        # device time per iteration with the host running ahead (events around the whole window), host issue per call
        host = []
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            host.append((time.perf_counter() - t0) * 1e3)
        e1.record()
        torch.cuda.synchronize()
        out[k] = {"ms_per_iter": round(e0.elapsed_time(e1) / n, 3), "host_issue": _stats(host),
                  "images_per_s": round(args.batch * n / e0.elapsed_time(e1) * 1e3, 1)}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(3):
            model.get_intermediate_layers(x, 4, return_class_token=True)
        e0, e1, _ = timed(lambda: [model.get_intermediate_layers(x, 4, return_class_token=True) for _ in range(10)])
    out["backbone_forward_ms"] = round(e0.elapsed_time(e1) / 10, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dim", type=int, default=1280)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--world", type=int, default=8, help="world size of the rate scaling: 8 gives the 52-classifier grid")
    ap.add_argument("--skip-backbone", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_probe: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "probe_alone": bench_probe_alone(args, dev)}
    if not args.skip_backbone:
        res["with_backbone"] = bench_with_backbone(args, dev)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
