"""DINOv2's multi-crop augmentation on one MI355X (csrc/dino_augment.hip, octic_vits_amd/dino_augment.py): B = 32 random uint8
sources of 375 x 500, the default geometry (2 x 224^2 + 8 x 96^2 crops per image).

  (a) the kernels alone: device time per batch between HIP events, warm, `--window` batches back to back per event pair, each
      batch with its own draw (tables uploaded in advance), against the bytes the batch needs: the sources' crop boxes and the
      coefficient pool read, the f32 crops written (what has to cross HBM), and with the uint8 intermediates between the four
      kernels counted as well (they are written and read once more; whether they stay in L2 / the Infinity Cache is not
      measured here).  Share of the 8.0 TB/s HBM peak for both.
  (b) the whole `apply`: draw, coefficient tables, upload and launches, host clock around a synchronise; and the host part alone.
  (c) what travels to the device per image (uint8 sources + tables) against the f32 crops.
  (d) where PIL imports: the same draws through the host oracle (tests/golden/dino_augment_case.py: real PIL calls, torch's
      conv2d for the blur, ToTensor + Normalize in numpy) on `--threads` host threads, in images/s.

    python tools/bench_dino_augment.py [--iters 20] [--window 8] [--out profiles/bench_dino_augment.txt]
Needs a GPU: there is no CPU path."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from octic_vits_amd.dino_augment import DinoAugment, pack_images  # noqa: E402

HBM_PEAK = 8.0e12


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def batch_bytes(params, tables):
    """(bytes that must cross HBM, bytes with the uint8 intermediates) of one batch."""
    boxes = params.box.reshape(-1, 4).astype(np.int64)
    src = int((boxes[:, 2] * boxes[:, 3] * 3).sum())
    B = len(params)
    crops = B * (2 * params.global_size ** 2 + params.n_local * params.local_size ** 2) * 3
    contrast = (params.jitter[..., None] & (params.order == 1)).any(-1)
    sizes = np.array([params.global_size] * 2 + [params.local_size] * params.n_local)[:, None] ** 2 * 3
    stats = int((contrast * sizes).sum())
    need = src + tables["coef"].nbytes + tables["rows_global"].nbytes + tables["rows_local"].nbytes + crops * 4
    return need, need + crops * 4 + stats                       # resize writes, jitter reads + writes, finish reads; statistics


def bench_pil(args, sources, aug):
    try:
        import PIL
    except ImportError:
        return None
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import dino_augment_case as C
    torch.set_num_threads(1)
    g = torch.Generator().manual_seed(3)
    imgs = sources[:args.pil_images]
    draws = [C.draw_image(im.shape[0], im.shape[1], generator=g) for im in imgs]
    mean, std = np.float32(aug.mean), np.float32(aug.std)

    def one(i):
        for p in draws[i]:
            out = C.apply_u8(imgs[i], p)
            ((out.astype(np.float32) / np.float32(255) - mean) / std).transpose(2, 0, 1).copy()

    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=args.threads) as ex:
        list(ex.map(one, range(len(imgs))))
    dt = time.perf_counter() - t0
    return PIL.__version__, len(imgs), len(imgs) / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--width", type=int, default=500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--pil-images", type=int, default=64)
    ap.add_argument("--step-ms", type=float, default=85.0, help="the SSL step at this batch to hold the figures against (README)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dino_augment: needs a GPU (no CPU path)")
    dev = torch.device("cuda")
    rs = np.random.RandomState(0)
    B = args.batch
    sources = [rs.randint(0, 256, (args.height, args.width, 3)).astype(np.uint8) for _ in range(max(B, args.pil_images))]
    aug = DinoAugment(generator=torch.Generator().manual_seed(1))
    packed = pack_images(sources[:B], dev)
    hs, ws = packed.host_sizes()

    # (a) kernels alone
    draws = [aug.draw(hs, ws) for _ in range(args.window)]
    host = [p.tables() for p in draws]
    tabs = [{k: torch.from_numpy(v).to(dev) for k, v in t.items()} for t in host]
    og = torch.empty(2 * B, 3, aug.global_crops_size, aug.global_crops_size, device=dev)
    ol = torch.empty(aug.local_crops_number * B, 3, aug.local_crops_size, aug.local_crops_size, device=dev)

    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for t in tabs:
            aug.launch(packed.data, t["rows_global"], t["rows_local"], t["coef"], out_global=og, out_local=ol)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.window

    for _ in range(args.warmup):
        window()
    ms = [window() for _ in range(args.iters)]
    need, with_mid = (float(np.mean(v)) for v in zip(*[batch_bytes(p, t) for p, t in zip(draws, host)]))
    med = _median(ms)

    # (b) the whole apply, and its host part
    for _ in range(2):
        aug.apply(packed)
    torch.cuda.synchronize()
    whole = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        aug.apply(packed)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    hostms = []
    for _ in range(args.iters):
        t0 = time.perf_counter()
        aug.draw(hs, ws).tables()
        hostms.append((time.perf_counter() - t0) * 1e3)

    # (c) the upload
    f32_per_image = (2 * aug.global_crops_size ** 2 + aug.local_crops_number * aug.local_crops_size ** 2) * 3 * 4
    table_bytes = float(np.mean([sum(v.nbytes for v in t.values()) for t in host]))
    up_per_image = (packed.data.numel() + table_bytes) / B

    lines = [
        f"device: {torch.cuda.get_device_name(0)}",
        f"batch {B} sources of {args.height} x {args.width} x 3 uint8, 2 x {aug.global_crops_size}^2 + {aug.local_crops_number} x {aug.local_crops_size}^2 crops per image, "
        f"{args.window} batches (own draws) per event pair, {args.iters} windows after {args.warmup} warm-up",
        f"kernels (8 launches): {med:.3f} ms per batch median (min {min(ms):.3f}, max {max(ms):.3f}) = {B / med * 1e3:.0f} images/s, {B * (2 + aug.local_crops_number) / med * 1e3:.0f} crops/s",
        f"bytes per batch: {need / 1e6:.1f} MB read + written across HBM at least (crop boxes, tables, f32 crops) = {need / med / 1e6:.0f} GB/s = {need / med * 1e3 / HBM_PEAK:.1%} of the 8.0 TB/s HBM peak;",
        f"                 {with_mid / 1e6:.1f} MB with the uint8 intermediates between the kernels = {with_mid / med / 1e6:.0f} GB/s = {with_mid / med * 1e3 / HBM_PEAK:.1%}",
        f"whole apply (draw + tables + upload + launches, host clock around a synchronise): {_median(whole):.2f} ms per batch median (min {min(whole):.2f}, max {max(whole):.2f});"
        f" host draw + coefficient tables alone: {_median(hostms):.2f} ms on one thread",
        f"upload per image: {up_per_image / 1e6:.3f} MB (uint8 source {packed.data.numel() / B / 1e6:.3f} MB + tables {table_bytes / B / 1e6:.3f} MB) against {f32_per_image / 1e6:.3f} MB of f32 crops"
        f" = {up_per_image / f32_per_image:.1%}",
        f"against the SSL step at this batch ({args.step_ms:.1f} ms): kernels {med / args.step_ms:.1%}, whole apply {_median(whole) / args.step_ms:.1%}, host draw + tables {_median(hostms) / args.step_ms:.1%}",
    ]
    pil = bench_pil(args, sources, aug)
    if pil is None:
        lines.append("host PIL chain: Pillow is not importable here, not measured")
    else:
        lines.append(f"host PIL oracle (Pillow {pil[0]}, {pil[1]} images, {args.threads} threads, ToTensor + Normalize in numpy): {pil[2]:.1f} images/s"
                     f" = {B / pil[2] * 1e3:.0f} ms per batch of {B}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
