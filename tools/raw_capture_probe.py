"""What a training step costs when the batch arrives as data.RawFrames -- the decoder's native-resolution frames, resized on the device --
on the metric configuration (16 videos x 2 clips x 2 frames, 2 captions per video of 32 tokens; the frames 360 x 640 RGB, interleaved, at
max_img_size 224), in ONE process:

  1. tasks.start_training eager on RawFrames                      (all that was possible before CapturedStep(raw_frames=True): the yardstick)
  2. tasks.start_training(capture=) with cfg.capture_raw_frames    (table check, descriptor upload, staging of text + table, replay)
  3. tasks.start_training(capture=) on square uint8 tensors        (the captured loop of tools/captured_loop_probe.py)

The three are timed in alternation, `--rounds` rounds of `--steps` optimizer steps each after a warm-up of every one (host clock around
a loop that ends in a device synchronise), and reported as the median / min / max per-step time over the rounds.  The stepper of 2 is
the object start_training(capture=True) builds from the config, kept over the windows.  2 minus 3 is set against the ingest launch
(profiles/yuv_ingest.txt: cb_resize_pack_u8 alone at this shape) and what 3 stages instead (the square frames); the descriptor upload and
the staging launch of 2 are timed between HIP events.  The loader is a list of device-resident batches of one signature.  Writes
profiles/raw_capture_loop.txt.  The process ends itself after --limit seconds.

    python tools/raw_capture_probe.py [--steps 300] [--rounds 5] [--out profiles/raw_capture_loop.txt]"""
import argparse
import copy
import faulthandler
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from clipbert_amd import captured as CAP  # noqa: E402
from clipbert_amd import data as D  # noqa: E402
from clipbert_amd import ops  # noqa: E402
from clipbert_amd import synthetic as S  # noqa: E402
from clipbert_amd import tasks  # noqa: E402
from clipbert_amd.bench import step as bench_step  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300, help="optimizer steps per timed window")
ap.add_argument("--rounds", type=int, default=5, help="windows per variant, alternating")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--videos", type=int, default=16)
ap.add_argument("--size", type=int, default=224)
ap.add_argument("--native", type=int, nargs=2, default=(360, 640), help="height and width of the decoder's frames")
ap.add_argument("--limit", type=int, default=420, help="seconds after which the process ends itself")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raw_capture_loop.txt"))
args = ap.parse_args()
faulthandler.dump_traceback_later(args.limit, exit=True)
assert torch.cuda.is_available(), "raw_capture_probe needs the GPU: a host timing says nothing about it"

st = bench_step.build(videos=args.videos, size=args.size)
model, opt, dev = st.model, st.opt, st.dev
h, w = args.native
n_b = 4                                                 # distinct batches of ONE signature, device-resident
raw, square = [], []
for i in range(n_b):
    ids, mask = S.synthetic_text(args.videos * 2, 32, 100 + i)
    text = dict(st.batch, text_input_ids=ids.to(dev), text_input_mask=mask.to(dev))
    g = torch.Generator().manual_seed(100 + i)
    videos = [torch.randint(0, 256, (4, h, w, 3), dtype=torch.uint8, generator=g) for _ in range(args.videos)]
    raw.append(dict(text, visual_inputs=D.collate_raw_frames(videos, args.size).to(dev)))
    square.append(dict(text, visual_inputs=S.synthetic_frames(args.videos, 4, args.size, 100 + i).to(dev)))
assert raw[0]["visual_inputs"].shape == square[0]["visual_inputs"].shape
raw_cfg = copy.copy(st.tcfg)
raw_cfg.capture_raw_frames = 1
# (the object start_training(capture=True) builds from this config, kept over the windows so that the graph is captured once)
steppers = {"raw captured": CAP.CapturedStep(model, opt, raw_cfg, raw_frames=bool(raw_cfg.capture_raw_frames)),
            "square captured": CAP.CapturedStep(model, opt, st.tcfg)}
loaders = {"raw eager": raw, "raw captured": raw, "square captured": square}
kinds = tuple(loaders)


def window(kind, steps):
    """`steps` optimizer steps of one variant -> seconds (host clock, device synchronised at both ends)"""
    cfg = copy.copy(raw_cfg if kind.startswith("raw") else st.tcfg)
    cfg.num_train_steps = steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = tasks.start_training(model, opt, loaders[kind], cfg, capture=steppers.get(kind, False))
    assert done == steps
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for k in kinds:
    window(k, max(args.warmup, 3))                      # sights 1 and 2 are eager, the graph exists from then on
for s in steppers.values():
    assert s.log[-1] == "replay" and s.stats["captures"] == 1 and s.stats["fallbacks"] == 0, (s.log, s.stats)
times = {k: [] for k in kinds}
for _ in range(args.rounds):
    for k in kinds:
        times[k].append(window(k, args.steps) / args.steps * 1e3)
for s in steppers.values():
    assert set(s.log[-args.steps:]) == {"replay"} and s.stats["captures"] == 1

# ---- what a replayed RawFrames step does before the replay ----------------------------------------------------------------------------
stepper = steppers["raw captured"]
entry = next(iter(stepper.graphs.values()))
rf = raw[0]["visual_inputs"]
table, host = rf.packed_table()
tensors = dict({k: v for k, v in raw[0].items() if torch.is_tensor(v)}, **{stepper.RAW_TABLE: table})
evs = []
for i in range(30):
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    e0.record()
    entry.source.point_at(raw[i % n_b]["visual_inputs"].flat)
    e1.record()
    stepper._stage(entry.bufs, tensors)
    e2.record()
    evs.append((e0, e1, e2))
torch.cuda.synchronize()
desc_us = sorted(a.elapsed_time(b) * 1e3 for a, b, _ in evs[5:])
stage_us = sorted(b.elapsed_time(c) * 1e3 for _, b, c in evs[5:])
stage_bytes = sum(v.numel() * v.element_size() for v in tensors.values())
sq_entry = next(iter(steppers["square captured"].graphs.values()))
sq_tensors = {k: v for k, v in square[0].items() if torch.is_tensor(v)}
evs = []
for i in range(30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    stepper._stage(sq_entry.bufs, sq_tensors)
    e1.record()
    evs.append((e0, e1))
torch.cuda.synchronize()
sq_stage_us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs[5:])
sq_stage_bytes = sum(v.numel() * v.element_size() for v in sq_tensors.values())
t0 = time.perf_counter()
for i in range(200):
    ops.resize_table_check(host, rf.n_frames, rf.flat.numel(), rf.max_img_size, rf.pixfmt)
check_us = (time.perf_counter() - t0) / 200 * 1e6
t0 = time.perf_counter()
for i in range(200):
    stepper._why_eager(raw[i % n_b])
    stepper.signature(raw[i % n_b])
sig_us = (time.perf_counter() - t0) / 200 * 1e6


def row(name, ms, unit="ms / step"):
    return f"{name:20s} median {statistics.median(ms):8.3f}  min {min(ms):8.3f}  max {max(ms):8.3f}  {unit}"


med = {k: statistics.median(v) for k, v in times.items()}
clips = st.clips_per_step
e_lo, e_hi = min(times["raw eager"]), max(times["raw eager"])
verdict = "2's median lies BELOW 1's whole min-max span" if med["raw captured"] < e_lo else \
    ("2's median lies INSIDE 1's min-max span: not faster beyond the spread" if med["raw captured"] <= e_hi else "2's median lies ABOVE 1's span: captured is SLOWER")
lines = [f"{torch.cuda.get_device_name(0)}; {args.videos} videos x 2 clips x 2 frames, RawFrames of {h} x {w} RGB (interleaved, {rf.flat.numel() / 1e6:.1f} MB per batch) at "
         f"max_img_size {args.size}, 2 captions x 32 tokens per video; {args.rounds} rounds of {args.steps} optimizer steps per variant, alternating, after warm-up; "
         "host clock around each window, device synchronised at both ends",
         row("1 raw eager", times["raw eager"]), row("2 raw captured", times["raw captured"]), row("3 square captured", times["square captured"]),
         f"clips/s at the medians: raw eager {clips / med['raw eager'] * 1e3:.0f}, raw captured {clips / med['raw captured'] * 1e3:.0f}, "
         f"square captured {clips / med['square captured'] * 1e3:.0f}",
         f"2 against 1: {med['raw eager'] / med['raw captured']:.2f} x  ({verdict})",
         f"2 minus 3: {(med['raw captured'] - med['square captured']) * 1e3:.0f} us per step; 2 runs the ingest launch + cb_stem_pool where 3 runs cb_stem_pool_u8 alone "
         "(profiles/yuv_ingest.txt: cb_resize_pack_u8 alone, this shape, 14.8 us), and stages less:",
         f"    2 descriptor upload (16 bytes, pinned -> device; HIP events): median {statistics.median(desc_us):.1f} us, min {desc_us[0]:.1f}, max {desc_us[-1]:.1f}",
         f"    2 staging launch (cb_copy_ranges, {len(tensors)} ranges, {stage_bytes / 1e3:.1f} KB; HIP events): median {statistics.median(stage_us):.1f} us, "
         f"min {stage_us[0]:.1f}, max {stage_us[-1]:.1f}",
         f"    3 staging launch (cb_copy_ranges, {len(sq_tensors)} ranges, {sq_stage_bytes / 1e6:.1f} MB; HIP events): median {statistics.median(sq_stage_us):.1f} us, "
         f"min {sq_stage_us[0]:.1f}, max {sq_stage_us[-1]:.1f}",
         f"    2 table check (cb_resize_table_check, {rf.n_frames} rows, host): {check_us:.1f} us; signature + fallback checks (host): {sig_us:.0f} us",
         "    loader: device-resident batches in all three, no share"]
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
