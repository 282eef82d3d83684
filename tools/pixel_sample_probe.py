"""What drawing the pixel sub-sampling on the device buys the pretraining loop, on the reference's own pretraining shape
(pretrain_image_text_base_resnet50_mlm_itm.json: 32 images of 768 px -> a 12 x 12 grid, Lv = 144; pixel_random_sampling_size 100;
30 text tokens; ~15 % of them labelled, mlm_capacity 256), in ONE process, ONE model, the same device-resident batches:

  1. pixel_sampling = "host",   tasks.start_training eager      (numpy draws + one H2D copy per forward: all the loop could do before)
  2. pixel_sampling = "device", tasks.start_training eager      (cb_pixel_sample, still launch by launch from Python)
  3. pixel_sampling = "device", tasks.start_training(capture=)  (the step replayed from its hipGraph, a fresh selection per replay)

timed in alternation, `--rounds` windows of `--steps` optimizer steps each after a warm-up of every variant (host clock around a loop
that ends in a device synchronise), reported as median / min / max per-step time over the windows.  Then cb_pixel_sample alone: a
hipGraph of 100 launches replayed between HIP events (per launch, so with the graph's node-to-node gap), at (144, 100) and (10000, 100).
Writes profiles/pixel_sample_loop.txt.  ``--kernel-only``: just 200 eager launches at (144, 100), for a kernel trace of their own.

    python tools/pixel_sample_probe.py [--steps 40] [--rounds 5] [--out profiles/pixel_sample_loop.txt]"""
import argparse
import copy
import faulthandler
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from clipbert_amd import captured as CAP  # noqa: E402
from clipbert_amd import modeling as M  # noqa: E402
from clipbert_amd import ops, tasks  # noqa: E402
from clipbert_amd import synthetic as S  # noqa: E402
from clipbert_amd.bench.step import BASE_CONFIG  # noqa: E402
from clipbert_amd.modeling.runtime import _SITE_PIXEL, _seed  # noqa: E402
from clipbert_amd.optim import FusedAdamW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40, help="optimizer steps per timed window")
ap.add_argument("--rounds", type=int, default=5, help="windows per variant, alternating")
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--images", type=int, default=32)
ap.add_argument("--size", type=int, default=768)
ap.add_argument("--sample", type=int, default=100)
ap.add_argument("--limit", type=int, default=420, help="seconds after which the process ends itself")
ap.add_argument("--kernel-only", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pixel_sample_loop.txt"))
args = ap.parse_args()
faulthandler.dump_traceback_later(args.limit, exit=True)
assert torch.cuda.is_available(), "pixel_sample_probe needs the GPU: a host timing says nothing about it"
dev = torch.device("cuda", 0)

if args.kernel_only:
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(100, dtype=torch.int32, device=dev)
    for _ in range(200):
        ops.pixel_sample(144, 100, _seed(_SITE_PIXEL), word, out=out)
        ops.counter_add(word)
    torch.cuda.synchronize()
    print("200 launches of cb_pixel_sample(144, 100); last selection starts", out[:6].tolist())
    sys.exit(0)

SEED, LT, CAP_SLOTS = 11, 30, 256
cfg = dict(BASE_CONFIG, attention_probs_dropout_prob=0.1, hidden_dropout_prob=0.1, pixel_random_sampling_size=args.sample, pixel_sampling="host")
model = M.ClipBert(cfg, detectron2_model_cfg="R-50-grid.yaml", transformer_cls=M.ClipBertForPreTraining)
model.load_state_dict(S.full_state_dict(cfg, "pretraining", SEED), strict=True)
model.to(dev).train(True)
model.prepare(dtype=torch.bfloat16, device=dev)
opt = FusedAdamW(model.rt.bank, lr=5e-5, betas=(0.9, 0.98), weight_decay=1e-3, max_grad_norm=5.0)
tcfg = argparse.Namespace(train_n_clips=1, num_frm=1, score_agg_func="mean", task=None, num_labels=2, gradient_accumulation_steps=1,
                          learning_rate=5e-5, cnn_learning_rate=5e-5, decay="linear", cnn_lr_decay="linear", num_train_steps=100000,
                          warmup_ratio=0.1, mlm_rows="labelled", mlm_capacity=CAP_SLOTS, use_mlm=1, use_itm=1, valid_steps=0,
                          train_batch_size=args.images)
batches = []
for i in range(4):                                      # distinct batches of ONE signature, device-resident
    g = torch.Generator().manual_seed(SEED + i)
    ids, mask = S.synthetic_text(args.images, LT, SEED + i)
    labels = torch.where((torch.rand(args.images, LT, generator=g) < 0.15) & (mask > 0), ids, torch.full_like(ids, -100))
    batches.append(dict(visual_inputs=S.synthetic_frames(args.images, 1, args.size, SEED + i).to(dev), text_input_ids=ids.to(dev),
                        text_input_mask=mask.to(dev), mlm_labels=labels.to(dev), itm_labels=torch.randint(0, 2, (args.images,), generator=g).to(dev),
                        n_examples_list=[1] * args.images))
with torch.no_grad():
    grid = model.grid_features(batches[0]["visual_inputs"])
lv = grid.shape[2] * grid.shape[3]
del grid
stepper = CAP.CapturedStep(model, opt, tcfg, loss_fn=tasks.pretrain_loss)
kinds = {"1 host, eager": ("host", False), "2 device, eager": ("device", False), "3 device, captured": ("device", stepper)}


def window(kind, steps):
    """`steps` optimizer steps of one variant -> seconds (host clock, device synchronised at both ends)"""
    mode, capture = kinds[kind]
    model.config.pixel_sampling = mode
    c = copy.copy(tcfg)
    c.num_train_steps = steps
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = tasks.start_training(model, opt, batches, c, capture=capture, loss_fn=tasks.pretrain_loss)
    torch.cuda.synchronize()
    assert done == steps
    return time.perf_counter() - t0


with warnings.catch_warnings(record=True) as caught:
    warnings.simplefilter("always")
    for k in kinds:
        window(k, max(args.warmup, 3))                  # (sights 1 and 2 of the captured variant are eager, the graph exists from then on)
    assert stepper.log[-1] == "replay" and stepper.stats["captures"] == 1 and stepper.stats["fallbacks"] == 0, (stepper.log, stepper.stats)
    times = {k: [] for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            times[k].append(window(k, args.steps) / args.steps * 1e3)
    assert set(stepper.log[-args.steps:]) == {"replay"}
assert not [w for w in caught if "runs eagerly" in str(w.message)], [str(w.message) for w in caught]
dropped = int(model.transformer.mlm_counts[1]) if getattr(model.transformer, "mlm_counts", None) is not None else -1


def kernel_us(lv_, n_):
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    out = torch.empty(n_, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            ops.pixel_sample(lv_, n_, _seed(_SITE_PIXEL), word, out=out)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(100):
            ops.pixel_sample(lv_, n_, _seed(_SITE_PIXEL), word, out=out)
    for _ in range(5):
        gr.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(7):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / 500 * 1e3)
    return us


k144, k10k = kernel_us(144, args.sample), kernel_us(10000, args.sample)


def row(name, ms):
    return f"{name:20s} median {statistics.median(ms):8.3f}  min {min(ms):8.3f}  max {max(ms):8.3f}  ms / step"


med = {k: statistics.median(v) for k, v in times.items()}
a, b, c = (med[k] for k in kinds)
lines = [f"{torch.cuda.get_device_name(0)}; pretraining (MLM + ITM), {args.images} images of {args.size} px (grid Lv = {lv}, {args.sample} pixels kept), {LT} text tokens, "
         f"labelled-rows MLM head with mlm_capacity {CAP_SLOTS} ({dropped} rows dropped over the run), dropout 0.1, bf16; {args.rounds} windows of {args.steps} optimizer "
         f"steps per variant, alternating, after warm-up; host clock around each window, device synchronised at both ends",
         *[row(k, times[k]) for k in kinds],
         f"3 against 1: {a / c:.3f} x  ({'captured is FASTER than the host-mode eager loop beyond the spread' if max(times['3 device, captured']) < min(times['1 host, eager']) else 'NOT faster beyond the spread'});"
         f"  2 against 1: {a / b:.3f} x",
         f"cb_pixel_sample alone, per launch inside a hipGraph of 100 launches (HIP events around 5 replays, 7 repeats; includes the node-to-node gap): "
         f"Lv 144, n {args.sample}: median {statistics.median(k144):.2f} us (min {min(k144):.2f}, max {max(k144):.2f});  "
         f"Lv 10000, n {args.sample}: median {statistics.median(k10k):.2f} us (min {min(k10k):.2f}, max {max(k10k):.2f})"]
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
