"""3-Augment on uint8 batches on one MI355X (csrc/augment.hip, octic_vits_amd/augment.py) at B = 64, 224 x 224.

  (a) the augmentation alone, device time between HIP events, warm, `--window` calls back to back per event pair: the recipe's
      own draws (a third of the samples each grayscale / solarize / blur, all with the full jitter), `to_tensor` (the identity
      table: ToTensor + Normalize only) and the worst table (every sample blurred, contrast last).  With the bytes the call
      needs (uint8 in, f32 out, the input once more for the samples with a contrast op) as achieved GB/s.
  (b) `--step MODEL`: the captured training step with the augmentation inside (`Trainer(mixup=, augment=)`, uint8 batches)
      against the same captured step fed pre-augmented f32 batches, windows of replays alternating in one process; a third
      arm replays the augmenting step with ONE table drawn in advance (no host draw per replay), which separates what the
      kernels cost inside the step from what the host's draw costs; `host_draw_ms` is that draw + table packing alone.
  (c) where PIL imports: the host chain the kernels replace (tests/golden/augment_case.py: real PIL calls + ToTensor +
      Normalize in numpy) in images/s on one core, for the record.

    python tools/bench_augment.py [--iters 30] [--window 20] [--step hybrid_deit_huge_patch14] [--out profiles/bench_augment.json]
Prints one JSON document.  Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octic_vits_amd.augment import AugParams, ThreeAugment  # noqa: E402
from octic_vits_amd.mixup import Mixup  # noqa: E402


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def _stats(us):
    return {"median_us": round(_median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2), "n": len(us)}


def _aug(seed):
    return ThreeAugment(rng=random.Random(seed), generator=torch.Generator().manual_seed(seed))


def bench_kernels(args, dev):
    B, H, W = args.batch, args.img, args.img
    g = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (B, H, W, 3), generator=g, device=dev, dtype=torch.uint8)
    out = torch.empty(B, 3, H, W, device=dev)
    aug = _aug(1)
    worst = AugParams.identity(B)
    worst.op[:], worst.radius[:], worst.order[:] = 3, 2.0, [0, 2, -1, 1]
    worst.brightness[:], worst.contrast[:], worst.saturation[:] = 1.2, 0.8, 1.1
    tables = {"recipe_draws": [aug.draw(B) for _ in range(args.window)], "to_tensor": [AugParams.identity(B)] * args.window,
              "all_blur_contrast_last": [worst] * args.window}
    dev_tables = {k: [torch.from_numpy(p.table()).to(dev) for p in v] for k, v in tables.items()}

    def window(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in dev_tables[k]:
            aug.launch(src, t, out=out)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.window

    for _ in range(args.warmup):
        for k in tables:
            window(k)
    res = {k: [] for k in tables}
    for _ in range(args.iters):                          # alternating: every table sees the same machine state
        for k in tables:
            res[k].append(window(k))
    doc = {"batch": B, "image": [H, W, 3], "window": args.window,
           "what": "us per call (statistics + output launch), device time, calls back to back between one event pair", "arms": {}}
    for k, ps in tables.items():
        contrast = np.mean([(p.order == 1).any(axis=1).mean() for p in ps])
        nbytes = src.numel() * (1 + contrast) + out.numel() * 4
        st = _stats(res[k])
        st["alg_MB"] = round(nbytes / 1e6, 1)
        st["GB_per_s"] = round(nbytes / st["median_us"] / 1e3, 1)
        st["blurred_share"] = round(float(np.mean([(p.op == 3).mean() for p in ps])), 3)
        doc["arms"][k] = st
    return doc


class _FixedDraw(ThreeAugment):
    """The first draw of a batch size again and again: the replay's host work without the draw."""

    def draw(self, B):
        if getattr(self, "_kept", None) is None or len(self._kept) != B:
            self._kept = super().draw(B)
        return self._kept


def bench_step(args, dev):
    from octic_vits_amd.deit_models import create_model
    from octic_vits_amd.train import Trainer
    nc, B = args.classes, args.batch
    g = torch.Generator(device=dev).manual_seed(2)
    batches = [(torch.randint(0, 256, (B, args.img, args.img, 3), generator=g, device=dev, dtype=torch.uint8),
                torch.randint(0, nc, (B,), generator=g, device=dev)) for _ in range(3)]
    pre = _aug(3)
    preaug = [(pre.apply(x), y) for x, y in batches]
    mix_kw = dict(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.0, num_classes=nc)
    arms = {}
    for name in ("augment_inside", "preaugmented_f32", "augment_inside_fixed_draw"):
        torch.manual_seed(0)
        model = create_model(args.step, num_classes=nc, drop_path_rate=0.5, img_size=args.img).to(dev)
        mix = Mixup(rng=np.random.RandomState(3), **mix_kw)
        if name == "augment_inside":
            arms[name] = (Trainer(model, mixup=mix, augment=_aug(3)).capture(*batches[0]), batches)
        elif name == "augment_inside_fixed_draw":
            fixed = _FixedDraw(rng=random.Random(3), generator=torch.Generator().manual_seed(3))
            arms[name] = (Trainer(model, mixup=mix, augment=fixed).capture(*batches[0]), batches)
        else:
            arms[name] = (Trainer(model, mixup=mix).capture(*preaug[0]), preaug)
    for gs, data in arms.values():
        for x, y in data:
            gs.replay(x, y)
    torch.cuda.synchronize()
    doc = {"model": args.step, "batch": B, "replays_per_window": args.step_window}
    samples, host = {k: [] for k in arms}, {k: [] for k in arms}
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
        doc[k] = {"ms_per_replay": {"median": round(_median(ms), 3), "min": round(ms[0], 3), "max": round(ms[-1], 3), "n": len(ms)},
                  "host_issue_ms": round(_median(host[k]), 3), "images_per_s": round(B / _median(ms) * 1e3, 1)}
    base = doc["preaugmented_f32"]["ms_per_replay"]["median"]
    doc["augment_inside_minus_preaugmented_ms"] = round(doc["augment_inside"]["ms_per_replay"]["median"] - base, 3)
    doc["fixed_draw_minus_preaugmented_ms"] = round(doc["augment_inside_fixed_draw"]["ms_per_replay"]["median"] - base, 3)
    aug = _aug(5)
    t0 = time.perf_counter()
    for _ in range(20):
        aug.draw(B).table()
    doc["host_draw_ms"] = round((time.perf_counter() - t0) / 20 * 1e3, 3)
    return doc


def bench_pil(args):
    """The per-sample host chain on ONE core: PIL ops, then ToTensor + Normalize in numpy."""
    try:
        import PIL
    except ImportError:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import augment_case
    torch.set_num_threads(1)
    rs = np.random.RandomState(0)
    rng, gen = random.Random(1), torch.Generator().manual_seed(1)
    imgs = rs.randint(0, 256, (args.pil_images, args.img, args.img, 3)).astype(np.uint8)
    params = [augment_case.draw_sample(rng=rng, generator=gen) for _ in range(len(imgs))]
    mean, std = np.float32([0.485, 0.456, 0.406]), np.float32([0.229, 0.224, 0.225])
    t0 = time.perf_counter()
    for px, p in zip(imgs, params):
        out = augment_case.apply_u8(px, p)
        ((out.astype(np.float32) / np.float32(255) - mean) / std).transpose(2, 0, 1).copy()
    dt = time.perf_counter() - t0
    return {"pillow": PIL.__version__, "images": len(imgs), "images_per_s_one_core": round(len(imgs) / dt, 1)}


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
    ap.add_argument("--pil-images", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    res = {"device": torch.cuda.get_device_name(0), "kernels": bench_kernels(args, dev)}
    if args.step:
        res["captured_step"] = bench_step(args, dev)
    pil = bench_pil(args)
    if pil is not None:
        res["host_pil_chain"] = pil
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
