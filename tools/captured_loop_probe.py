"""What the task loop costs per step against the captured step the benchmark replays, on the metric configuration (16 videos x 2 clips x
2 frames of 224 px, 2 captions per video of 32 tokens), in ONE process:

  1. tasks.start_training eager                     (every launch through ctypes + autograd from Python: what the loop did before capture=)
  2. tasks.start_training(capture=CapturedStep)     (stage the batch, prepare_step, replay)
  3. the clipbert_amd.bench.step graph on its fixed batch (host_prepare + replay: what bench.py times)

The three are timed in alternation, `--rounds` rounds of `--steps` optimizer steps each after a warm-up of every one (host clock around
a loop that ends in a device synchronise), and reported as the median / min / max per-step time over the rounds.  The gap between 2 and
3 is attributed: the staging launch (HIP events around cb_copy_ranges on the batch), the host time of the signature + fallback checks,
and the remainder (Python of step(), the loss clone); prepare_step is in both.  The loader is a list of device-resident batches of one
signature (a PrefetchLoader delivers batches the same way: already in HBM), so it contributes nothing to either loop here.

Then the 16-clip retrieval inference row (one video x 16 clips against 64 captions per mini-batch, 4 mini-batches): tasks.
inference_retrieval_video eager against capture=.  Writes profiles/captured_loop.txt.  The process ends itself after --limit seconds.

    python tools/captured_loop_probe.py [--steps 300] [--rounds 5] [--out profiles/captured_loop.txt]"""
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
ap.add_argument("--limit", type=int, default=420, help="seconds after which the process ends itself")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "captured_loop.txt"))
args = ap.parse_args()
faulthandler.dump_traceback_later(args.limit, exit=True)
assert torch.cuda.is_available(), "captured_loop_probe needs the GPU: a host timing says nothing about it"

st = bench_step.build(videos=args.videos, size=args.size)
model, opt, dev = st.model, st.opt, st.dev
n_b = 4                                                 # distinct batches of ONE signature, device-resident
batches = []
for i in range(n_b):
    ids, mask = S.synthetic_text(args.videos * 2, 32, 100 + i)
    batches.append(dict(st.batch, visual_inputs=S.synthetic_frames(args.videos, 4, args.size, 100 + i).to(dev), text_input_ids=ids.to(dev),
                        text_input_mask=mask.to(dev)))
stepper = CAP.CapturedStep(model, opt, st.tcfg)
graph = None


def window(kind, steps):
    """`steps` optimizer steps of one variant -> seconds (host clock, device synchronised at both ends)"""
    cfg = copy.copy(st.tcfg)
    cfg.num_train_steps = steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if kind == "bench graph":
        for _ in range(steps):
            st.host_prepare()
            graph.replay()
    else:
        done = tasks.start_training(model, opt, batches, cfg, capture=stepper if kind == "loop captured" else False)
        assert done == steps
    torch.cuda.synchronize()
    return time.perf_counter() - t0


kinds = ("loop eager", "loop captured", "bench graph")
window("loop eager", args.warmup)
window("loop captured", max(args.warmup, 3))            # sights 1 and 2 are eager, the graph exists from then on
assert stepper.log[-1] == "replay" and stepper.stats["captures"] == 1, (stepper.log, stepper.stats)
graph, _ = st.capture()
window("bench graph", args.warmup)
times = {k: [] for k in kinds}
for _ in range(args.rounds):
    for k in kinds:
        times[k].append(window(k, args.steps) / args.steps * 1e3)
assert set(stepper.log[-args.steps:]) == {"replay"}

# ---- the gap between the captured loop and the bench graph ---------------------------------------------------------------------
entry = next(iter(stepper.graphs.values()))
tensors = {k: v for k, v in batches[0].items() if torch.is_tensor(v)}
evs = []
for i in range(30):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    stepper._stage(entry.bufs, tensors)
    e1.record()
    evs.append((e0, e1))
torch.cuda.synchronize()
stage_us = sorted(a.elapsed_time(b) * 1e3 for a, b in evs[5:])
stage_bytes = sum(v.numel() * v.element_size() for v in tensors.values())
t0 = time.perf_counter()
for i in range(200):
    stepper._why_eager(batches[i % n_b])
    stepper.signature(batches[i % n_b])
sig_us = (time.perf_counter() - t0) / 200 * 1e6
t0 = time.perf_counter()
for i in range(50):
    tasks.set_learning_rates(opt, st.tcfg, i + 1)
    opt.prepare_step()
torch.cuda.synchronize()
prep_us = (time.perf_counter() - t0) / 50 * 1e6

# ---- retrieval inference: one video x 16 clips, 4 mini-batches of 64 captions ----------------------------------------------------
icfg = copy.copy(st.tcfg)
icfg.inference_n_clips, icfg.num_frm, icfg.inference_batch_size = 16, 2, 64
vis = S.synthetic_frames(1, 32, args.size, 9).to(dev)
ids, mask = (t.to(dev) for t in S.synthetic_text(256, 32, 9))
model.eval()
cf = CAP.CapturedForward(model)


def infer(capture, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        scores = tasks.inference_retrieval_video(model, vis, ids, mask, icfg, capture=capture)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, scores


_, want = infer(None, 2)
_, got = infer(cf, 2)
assert cf.log[-1] == "replay" and got == want, "captured inference scores differ from the eager ones"
itimes = {"inference eager": [], "inference captured": []}
for _ in range(args.rounds):
    itimes["inference eager"].append(infer(None, 20)[0])
    itimes["inference captured"].append(infer(cf, 20)[0])
model.train(True)


def row(name, ms, unit="ms / step"):
    return f"{name:20s} median {statistics.median(ms):8.3f}  min {min(ms):8.3f}  max {max(ms):8.3f}  {unit}"


med = {k: statistics.median(v) for k, v in times.items()}
clips = st.clips_per_step
lines = [f"{torch.cuda.get_device_name(0)}; {args.videos} videos x 2 clips x 2 frames of {args.size} px, 2 captions x 32 tokens per video; {args.rounds} rounds of "
         f"{args.steps} optimizer steps per variant, alternating, after warm-up; host clock around each window, device synchronised at both ends",
         row("1 loop eager", times["loop eager"]), row("2 loop captured", times["loop captured"]), row("3 bench graph", times["bench graph"]),
         f"clips/s at the medians: eager {clips / med['loop eager'] * 1e3:.0f}, captured {clips / med['loop captured'] * 1e3:.0f}, bench graph {clips / med['bench graph'] * 1e3:.0f}",
         f"2 against 1: {med['loop eager'] / med['loop captured']:.2f} x  ({'captured is FASTER' if med['loop captured'] < min(times['loop eager']) else 'captured is NOT faster beyond the spread'})",
         f"2 minus 3: {(med['loop captured'] - med['bench graph']) * 1e3:.0f} us per step, of which",
         f"    staging launch (cb_copy_ranges, {len(tensors)} ranges, {stage_bytes / 1e6:.1f} MB; HIP events): median {statistics.median(stage_us):.1f} us, min {stage_us[0]:.1f}, max {stage_us[-1]:.1f}"
         f"  ({2 * stage_bytes / statistics.median(stage_us) / 1e6:.2f} TB/s read + written)",
         f"    signature + fallback checks (host): {sig_us:.0f} us",
         f"    the rest is Python of step() / start_training and the loss clone; set_learning_rates + prepare_step (host, {prep_us:.0f} us) is in 2 AND 3",
         "    loader: device-resident batches in both loops, no share",
         row("inference eager", itimes["inference eager"], "ms / video (16 clips x 256 captions)"),
         row("inference captured", itimes["inference captured"], "ms / video (16 clips x 256 captions)"),
         f"inference captured against eager: {statistics.median(itimes['inference eager']) / statistics.median(itimes['inference captured']):.2f} x; scores equal"]
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
