"""The DeiT-III crops and the evaluation resize on one MI355X (csrc/crop.hip, octic_vits_amd/crop.py): B = 64 random uint8 sources
of 375 x 500, output 224 x 224.

  (a) RandomResizedCrop mode, uint8 out: the windowed kernel (octic_crop_resize_u8) against the multi-crop resize kernel
      (octic_dino_resize_u8) on the SAME boxes and coefficients, drawn by ``crop.RandomResizedCrop``.  Device time between HIP
      events, warm, `--window` launches back to back per event pair, the two arms alternating in one process, `--iters` pairs each
      (every pair with its own draw, tables uploaded in advance); median and the spread of the repeats.  Bytes that must cross
      HBM: the boxes' source bytes, the tables, the output; GB/s and the share of the 8.0 TB/s HBM peak for both.
  (b) evaluation mode (Resize(256) + CenterCrop(224)): f32 NCHW in ONE launch against uint8 out followed by
      ``augment.to_tensor``.
  (c) where PIL imports: the draws of (a) through ``img.crop(box).resize((224, 224), BICUBIC)`` on `--threads` host threads.
  (d) bytes uploaded per image: the packed source against the 224 x 224 x 3 crop as uint8 and as f32.

    python tools/bench_crop.py [--iters 20] [--window 8] [--out profiles/bench_crop.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octic_vits_amd import augment, ops  # noqa: E402
from octic_vits_amd.crop import EvalTransform, RandomResizedCrop  # noqa: E402
from octic_vits_amd.dino_augment import DinoAugParams, pack_images  # noqa: E402

HBM_PEAK = 8.0e12


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def timed(fn, window):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(window):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / window


def bench_pil(args, sources, boxes, S):
    try:
        import PIL
        from PIL import Image
    except ImportError:
        return None
    n = min(args.pil_images, len(sources))
    imgs = [Image.fromarray(s) for s in sources[:n]]

    def one(i):
        t, l, h, w = (int(v) for v in boxes[i])
        np.asarray(imgs[i].crop((l, t, l + w, t + h)).resize((S, S), Image.BICUBIC))

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=args.threads) as ex:
        for _ in range(args.pil_repeats):
            list(ex.map(one, range(n)))
    return PIL.__version__, n * args.pil_repeats, n * args.pil_repeats / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pil-images", type=int, default=64)
    ap.add_argument("--pil-repeats", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_crop: needs a GPU (the kernels have no CPU path)")
    dev, B, S = "cuda", args.batch, args.size
    rs = np.random.RandomState(0)
    sources = [rs.randint(0, 256, (args.height, args.width, 3)).astype(np.uint8) for _ in range(B)]
    packed = pack_images(sources, dev)
    hs, ws = packed.host_sizes()
    lines = [f"bench_crop: B {B} sources of {args.height} x {args.width}, output {S} x {S}, {args.iters} x {args.window} launches per arm, "
             f"{torch.cuda.get_device_name(0)}"]

    # ---- (a) RandomResizedCrop: the windowed kernel against the multi-crop resize kernel, the same boxes and coefficients
    rrc = RandomResizedCrop(size=S, rng=random.Random(1))
    draws = []
    for _ in range(args.iters):
        p = rrc.draw(hs, ws)
        t = p.tables()
        box2 = np.stack([p.box, p.box])
        d = DinoAugParams(hs, ws, 0, S, S, box=box2).tables()
        need = int((p.box[:, 2].astype(np.int64) * p.box[:, 3] * 3).sum()) + B * S * S * 3
        draws.append(dict(params=p, rows=torch.from_numpy(t["rows"]).to(dev), coef=torch.from_numpy(t["coef"]).to(dev),
                          drows=torch.from_numpy(np.ascontiguousarray(d["rows_global"][:B])).to(dev), dcoef=torch.from_numpy(d["coef"]).to(dev),
                          bytes_new=need + t["rows"].nbytes + t["coef"].nbytes,
                          bytes_old=need + d["rows_global"][:B].nbytes + d["coef"].nbytes))
    out_new = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    out_old = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    new = lambda d: ops.crop_resize_u8(packed.data, d["rows"], d["coef"], rrc.mean, rrc.std, out_new)
    old = lambda d: ops.dino_resize_u8(packed.data, d["drows"], d["dcoef"], S, out_old)
    for d in draws[:3]:                                        # warm, and the two kernels agree bit for bit
        new(d), old(d)
        assert torch.equal(out_new, out_old)
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for d in draws:                                            # alternating arms
        t_new.append(timed(lambda: new(d), args.window))
        t_old.append(timed(lambda: old(d), args.window))
    for name, ts, key in (("octic_crop_resize_u8 (new)", t_new, "bytes_new"), ("octic_dino_resize_u8 (parent)", t_old, "bytes_old")):
        med, lo, hi = stats(ts)
        nbytes = float(np.mean([d[key] for d in draws]))
        lines.append(f"(a) RRC uint8   {name:32s} {med * 1e3:8.1f} us per batch (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), {nbytes / 1e6:.2f} MB "
                     f"-> {nbytes / med / 1e6:.1f} GB/s, {100 * nbytes / (med * 1e-3) / HBM_PEAK:.2f} % of the HBM peak, "
                     f"{B / med * 1e3:.0f} images/s")
    lines.append(f"(a) new / parent time {stats(t_new)[0] / stats(t_old)[0]:.3f} (median of per-draw ratios "
                 f"{stats([a / b for a, b in zip(t_new, t_old)])[0]:.3f})")

    # ---- (b) evaluation: f32 in one launch against uint8 + to_tensor
    ev = EvalTransform(size=S)
    p = ev.draw(hs, ws)
    t = ev.upload(p.tables(), dev)
    f32 = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    f32b = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
    one = lambda: ev.launch(packed.data, t["rows"], t["coef"], out=f32)
    two = lambda: augment.to_tensor(ev.launch(packed.data, t["rows"], t["coef"], out=u8, uint8_out=True), out=f32b)
    one(), two()
    assert torch.equal(f32, f32b)
    torch.cuda.synchronize()
    t_one, t_two, t_u8 = [], [], []
    for _ in range(args.iters):
        t_one.append(timed(one, args.window))
        t_two.append(timed(two, args.window))
        t_u8.append(timed(lambda: ev.launch(packed.data, t["rows"], t["coef"], out=u8, uint8_out=True), args.window))
    src_bytes = int(hs @ ws) * 3
    for name, ts, nbytes in (("f32 NCHW, one launch", t_one, src_bytes + B * S * S * 12), ("uint8 NHWC, one launch", t_u8, src_bytes + B * S * S * 3),
                             ("uint8 + augment.to_tensor", t_two, src_bytes + B * S * S * (3 + 3 + 12))):
        med, lo, hi = stats(ts)
        lines.append(f"(b) eval        {name:32s} {med * 1e3:8.1f} us per batch (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}), {nbytes / 1e6:.2f} MB "
                     f"-> {nbytes / med / 1e6:.1f} GB/s, {100 * nbytes / (med * 1e-3) / HBM_PEAK:.2f} % of the HBM peak, {B / med * 1e3:.0f} images/s")

    # ---- the whole apply (draw, tables, upload, launch), host clock around a synchronise
    for name, fn in (("RandomResizedCrop.apply (uint8)", lambda: rrc.apply(packed, uint8_out=True)), ("EvalTransform.apply (f32)", lambda: ev.apply(packed))):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.iters):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        med, lo, hi = stats(ts)
        lines.append(f"    whole       {name:32s} {med:8.3f} ms per batch (min {lo:.3f}, max {hi:.3f}): draw, coefficient tables, upload, launch")

    # ---- (c) PIL on host threads
    pil = bench_pil(args, sources, draws[0]["params"].box, S)
    lines.append("(c) PIL absent" if pil is None else
                 f"(c) PIL {pil[0]}: {pil[1]} crops, img.crop(box).resize(({S}, {S}), BICUBIC) on {args.threads} host threads: {pil[2]:.0f} images/s")

    # ---- (d) the upload
    per = src_bytes / B
    tables = (draws[0]["rows"].numel() + draws[0]["coef"].numel()) * 4 / B
    lines.append(f"(d) upload per image: packed source {per / 1e6:.3f} MB (+ {tables:.0f} B of tables in RRC mode) "
                 f"against {S * S * 3 / 1e6:.3f} MB for the uint8 crop and {S * S * 12 / 1e6:.3f} MB for the f32 crop: "
                 f"{per / (S * S * 3):.2f} x the uint8 crop, {per / (S * S * 12):.2f} x the f32 crop")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
