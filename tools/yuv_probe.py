"""YUV 4:2:0 ingest: time cb_resize_pack_yuv420 against cb_resize_pack_u8 on the same pictures, in the same run.

For 64 frames of 360 x 640 -> 224 and 64 frames of 720 x 1280 -> 448 (bf16 output, pad 3, 2 extra columns: the training configuration):
random I420 planes, the same planes as NV12, and the interleaved uint8 RGB frames they stand for (tests/yuv_restatement.py, BT.601
limited -- what the loader would have shipped after the decoder's to_rgb()).  The three launches are timed INTERLEAVED: --reps (30) rounds,
each round one sample per launch, a sample being HIP events around --inner (20) back-to-back launches / inner, after a warm-up.  Medians
and ranges; the yardstick is the u8 kernel of THIS run, never a number from elsewhere.  The outputs are compared byte for byte first
(the definition of the entry point, at the sizes that are timed).  Bytes shipped per batch (pinned buffer, host-to-device copy) are
computed from the shapes, not measured.

    python tools/yuv_probe.py [--out profiles/yuv_ingest.txt] [--reps 30] [--inner 20]
Writes the table (with its command line) to --out and prints it."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import yuv_restatement as Y  # noqa: E402
from clipbert_amd import data, ops  # noqa: E402
from clipbert_amd import synthetic as S  # noqa: E402

CASES = [(64, 360, 640, 224), (64, 720, 1280, 448)]
MATRIX = "bt601"


def pictures(n, h, w, seed):
    """n random pictures as I420 frames, NV12 frames (n, frame_bytes) and interleaved RGB frames (n, h, w, 3)"""
    i420, nv12, rgb = [], [], []
    for k in range(n):
        planes = Y.random_planes(h, w, seed + k)
        i420.append(Y.pack(*planes, "i420"))
        nv12.append(Y.pack(*planes, "nv12"))
        rgb.append(Y.planes_to_rgb(*planes, MATRIX).transpose(1, 2, 0))
    return (torch.from_numpy(np.stack(a)) for a in (i420, nv12, rgb))


def sample_us(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"YUV 4:2:0 ingest: cb_resize_pack_yuv420 against cb_resize_pack_u8 on the same pictures ({torch.cuda.get_device_name(0)})",
             " ".join(["python", "tools/yuv_probe.py"] + sys.argv[1:]),
             f"bf16 output, pad 3, extra_w 2, matrix {MATRIX}; {args.reps} interleaved samples per launch, a sample = {args.inner} back-to-back launches / {args.inner}; us, median (min..max)",
             ""]
    all_equal = True
    for n, h, w, size in CASES:
        i420, nv12, rgb = pictures(n, h, w, 1000 * size)
        frames = {"u8 rgb (h, w, 3)": data.collate_raw_frames([rgb], size, hwc=True), "yuv420 i420": data.collate_yuv_frames([(i420, h, w)], size, "i420", MATRIX),
                  "yuv420 nv12": data.collate_yuv_frames([(nv12, h, w)], size, "nv12", MATRIX)}
        runs, outs = {}, {}
        for name, rf in frames.items():
            rf = rf.to(dev)
            table, host = rf.packed_table()
            if rf.pixfmt == "rgb":
                runs[name] = lambda rf=rf, table=table, host=host: ops.resize_pack_u8(rf.flat, table, n, size, torch.bfloat16, S.PIXEL_MEAN, S.PIXEL_STD, hwc=True,
                                                                                      pad=3, extra_w=2, host_table=host)
            else:
                runs[name] = lambda rf=rf, table=table, host=host: ops.resize_pack_yuv420(rf.flat, table, n, size, torch.bfloat16, S.PIXEL_MEAN, S.PIXEL_STD,
                                                                                          layout=rf.pixfmt, matrix=rf.matrix, pad=3, extra_w=2, host_table=host)
            outs[name] = runs[name]()
        torch.cuda.synchronize()
        ref = outs["u8 rgb (h, w, 3)"].view(torch.int16)
        equal = {name: bool(torch.equal(o.view(torch.int16), ref)) for name, o in outs.items()}
        all_equal = all_equal and all(equal.values())
        for _ in range(3):
            for fn in runs.values():
                sample_us(fn, args.inner)
        times = {name: [] for name in runs}
        for _ in range(args.reps):
            for name, fn in runs.items():
                times[name].append(sample_us(fn, args.inner))
        base = statistics.median(times["u8 rgb (h, w, 3)"])
        lines.append(f"{n} frames of {h} x {w} -> {size}  (packed image written: {outs['yuv420 i420'].numel() * 2 / 1e6:.1f} MB)")
        for name, rf in frames.items():
            med = statistics.median(times[name])
            lines.append(f"  {name:18s} {med:8.1f} ({min(times[name]):.1f}..{max(times[name]):.1f}) us   {med / base:5.2f} x u8   "
                         f"bytes shipped per batch (computed) {rf.flat.numel():>10d} = {rf.flat.numel() / (n * h * w):.2f} B/px   "
                         f"output == u8 output: {equal[name]}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    if not all_equal:
        sys.exit("outputs differ")


if __name__ == "__main__":
    main()
