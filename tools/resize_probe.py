"""Raw-frame ingest: time cb_resize_pack_u8 against the only route the library offered before it for native-resolution frames.

For 64 frames of 360 x 640 -> 224 and 16 frames of 720 x 1280 -> 448 (uint8, interleaved):
  (a) the one launch ops.resize_pack_u8 (bf16 output, the training configuration): HIP events around a batch of launches, warm, median
      of >= 20 repeats; bytes moved (source frames once + packed image) / time against the 8 TB/s HBM peak and the 6.3 TB/s a streaming
      copy reaches (tools/hbm_table.py);
  (b) host resize: F.interpolate (bilinear, 16 threads) + F.pad + ImageNorm on the fp32 frames (wall clock), then the pinned fp32 H2D
      copy + ops.stem_pack of the normalised frames (HIP events).
The GB/s column counts every source byte ONCE: it assumes that the 4 taps of a pixel, which neighbouring threads share, are served from
the caches; when downscaling by more than 2 some source bytes are never read at all, so it is an upper bound on the traffic.

    python tools/resize_probe.py [--out profiles/NAME.md] [--reps 20]
Writes a markdown table (with its command line) to --out and prints it."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from clipbert_amd import data, ops  # noqa: E402
from clipbert_amd import synthetic as S  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12
CASES = [(64, 360, 640, 224), (16, 720, 1280, 448)]


def gpu_us(fn, reps, inner=10):
    """median over ``reps`` of (HIP-event time of ``inner`` back-to-back calls) / inner, after a warm-up"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / inner)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_num_threads(16)
    lines = [f"# Raw-frame ingest: resize + pad + ImageNorm on the GPU vs on the host ({torch.cuda.get_device_name(0)})", "",
             "`" + " ".join(["python", "tools/resize_probe.py"] + sys.argv[1:]) + "`", "",
             "| frames | (a) cb_resize_pack_u8 us (min..max) | MB moved (source once + packed image) | GB/s | % of 8 TB/s | % of 6.3 TB/s copy | (b) host F.interpolate+pad+norm ms | "
             "(b) fp32 H2D + stem_pack us | (b) total ms | (b) / (a) |", "|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for n, h, w, size in CASES:
        g = torch.Generator().manual_seed(n)
        frames = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        rf = data.collate_raw_frames([frames], size, hwc=True).to(dev)
        table, host = rf.packed_table()
        run = lambda: ops.resize_pack_u8(rf.flat, table, n, size, torch.bfloat16, S.PIXEL_MEAN, S.PIXEL_STD, hwc=True, pad=3, extra_w=2,
                                         host_table=host)
        packed = run()
        med, lo, hi = gpu_us(run, args.reps)
        moved = rf.flat.numel() + packed.numel() * packed.element_size()
        # (b) the host route: planar float frames as the reference's dataset holds them
        nh, nw = data.resize_size(h, w, size)
        planar = frames.permute(0, 3, 1, 2).contiguous()
        mean, std = torch.tensor(S.PIXEL_MEAN).view(1, 3, 1, 1), torch.tensor(S.PIXEL_STD).view(1, 3, 1, 1)
        host_ms = []
        for _ in range(max(3, args.reps // 4)):
            t0 = time.perf_counter()
            x = F.pad(F.interpolate(planar.float(), size=(nh, nw), mode="bilinear", align_corners=False), (0, size - nw, 0, size - nh))
            x.sub_(mean).div_(std)
            host_ms.append((time.perf_counter() - t0) * 1e3)
        pinned = torch.empty(x.shape, dtype=torch.float32).pin_memory()
        pinned.copy_(x)
        route_b = lambda: ops.stem_pack(pinned.to(dev, non_blocking=True), torch.bfloat16, 3, extra_w=2)
        b_med, _, _ = gpu_us(route_b, args.reps, inner=2)
        b_total = statistics.median(host_ms) + b_med / 1e3
        bw = moved / (med * 1e-6)
        lines.append(f"| {n} x {h} x {w} -> {size} | {med:.1f} ({lo:.1f}..{hi:.1f}) | {moved / 1e6:.1f} | {bw / 1e9:.0f} | {100 * bw / HBM_PEAK:.0f} | "
                     f"{100 * bw / HBM_COPY:.0f} | {statistics.median(host_ms):.1f} | {b_med:.0f} | {b_total:.1f} | {b_total * 1e3 / med:.0f}x |")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
