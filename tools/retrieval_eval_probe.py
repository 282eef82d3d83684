#!/usr/bin/env python
"""Retrieval evaluation, the dict-row path against the device path, both from THIS tree, on one MI355X (profiles/retrieval_eval.md):

  metrics stage   a synthetic 1000 x 1000 score matrix (MSRVTT 1k-A): tasks.eval_retrieval over the 10^6 dict rows against
                  tasks.eval_retrieval_matrix (two cb_retrieval_rank launches, one copy back);
  whole loop      32 videos x 256 captions, 4 clips x 2 frames at 224 px, bf16 model of full size, inference_batch_size 64,
                  capture=True: tasks.inference_retrieval against tasks.inference_retrieval_matrix + tasks.eval_retrieval_matrix.

One warm-up per arm, then --repeats timed runs per arm, the arms alternating; host clock around a device synchronise on both sides.
Prints a markdown table (all runs sorted, the median) and, with --out, writes it to a file.  Not the headline metric (bench.py is)."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import bench
from clipbert_amd import modeling as M, synthetic as S, tasks
from oracle import clipbert_oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--n", type=int, default=1000, help="videos = captions of the metrics stage")
ap.add_argument("--videos", type=int, default=32)
ap.add_argument("--captions", type=int, default=256)
ap.add_argument("--clips", type=int, default=4)
ap.add_argument("--out", default="", help="also write the table to this file")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("retrieval_eval_probe: no GPU visible (a timing on the host says nothing about the device)")
dev = torch.device("cuda", 0)


def timed(arms, repeats):
    """arms: {name: callable}; one warm-up each, then the arms alternating -> {name: seconds per run, sorted}"""
    for fn in arms.values():
        fn()
    out = {name: [] for name in arms}
    for _ in range(repeats):
        for name, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[name].append(time.perf_counter() - t0)
    return {name: sorted(v) for name, v in out.items()}


def row(stage, arm, secs):
    ms = [1e3 * s for s in secs]
    return f"| {stage} | {arm} | {' '.join(f'{m:.2f}' for m in ms)} | {statistics.median(ms):.2f} | {ms[0]:.2f} - {ms[-1]:.2f} |"


lines = ["| stage | arm | ms per run, sorted | median ms | min - max ms |", "|---|---|---|---:|---|"]
notes = []

# ---- metrics stage ------------------------------------------------------------------------------------------------------------------
n = args.n
rng = np.random.default_rng(0)
logits = rng.normal(0.0, 6.0, (n, n)).astype(np.float32)
logits[np.arange(n), np.arange(n)] += 6.0                    # the ground truth mostly ahead, most scores saturated: ties as in a real run
scores = torch.sigmoid(torch.from_numpy(logits)).to(dev)
vid_ids, txt_ids = [f"video{i}" for i in range(n)], [f"cap{j}" for j in range(n)]
gt = {t: v for t, v in zip(txt_ids, vid_ids)}
matrix = tasks.RetrievalMatrix(vid_ids, txt_ids, scores)
t0 = time.perf_counter()
rows = tasks.retrieval_rows(matrix)
notes.append(f"building the {len(rows)} dict rows from the matrix (not part of either arm): {time.perf_counter() - t0:.2f} s")
res = {}
t = timed({"eval_retrieval (dict rows)": lambda: res.__setitem__("old", tasks.eval_retrieval(rows, gt)),
           "eval_retrieval_matrix": lambda: res.__setitem__("new", tasks.eval_retrieval_matrix(matrix, gt))}, args.repeats)
for name, secs in t.items():
    lines.append(row(f"metrics, {n} x {n}", f"`{name}`", secs))
keys = np.rint(scores.cpu().numpy().astype(np.float64) * 1e4)
notes.append(f"metrics stage: {int(keys.size - sum(len(np.unique(r)) for r in keys))} of {keys.size} rounded scores repeat another one of their row")
notes.append(f"metrics stage, dict rows (torch.sort without stable=True): {res['old']}")
notes.append(f"metrics stage, matrix (stable order): {res['new']}")
del rows

# ---- whole loop ---------------------------------------------------------------------------------------------------------------------
cfg = dict(bench.BASE_CONFIG)
model = M.ClipBert(cfg, detectron2_model_cfg="R-50-grid.yaml", transformer_cls=M.ClipBertForVideoTextRetrieval)
model.load_state_dict(S.full_state_dict(cfg, "retrieval", 42), strict=True)
model.to(dev).eval()
model.prepare(dtype=torch.bfloat16, device=dev)
icfg = SimpleNamespace(inference_n_clips=args.clips, num_frm=2, score_agg_func="lse", inference_batch_size=64)
ids, mask = S.synthetic_text(args.captions, 32, 42)
ids, mask = ids.to(dev), mask.to(dev)
cap_ids = [f"cap{j}" for j in range(args.captions)]
videos = []
for i in range(args.videos):
    vis = O.image_norm(S.synthetic_frames(1, args.clips * 2, 224, 100 + i), S.PIXEL_MEAN, S.PIXEL_STD).to(dev)
    videos.append(dict(vid_id=f"video{i}", visual_inputs=vis, text_input_ids=ids, text_input_mask=mask, caption_ids=cap_ids))
gt = {t: f"video{j % args.videos}" for j, t in enumerate(cap_ids)}


def old_loop():
    res["old_rows"], res["old_metrics"] = tasks.inference_retrieval(model, videos, icfg, gt, capture=True)


def new_loop():
    res["matrix"] = tasks.inference_retrieval_matrix(model, videos, icfg, capture=True)
    res["new_metrics"] = tasks.eval_retrieval_matrix(res["matrix"], gt)


stage = f"loop, {args.videos} videos x {args.captions} captions x {args.clips} clips"
t = timed({"inference_retrieval": old_loop, "inference_retrieval_matrix + eval_retrieval_matrix": new_loop}, args.repeats)
for name, secs in t.items():
    lines.append(row(stage, f"`{name}`", secs))
new_keys = np.rint(res["matrix"].scores.cpu().numpy().astype(np.float64) * 1e4).astype(np.int64).reshape(-1)
old_keys = np.array([int(np.rint(1e4 * r["score"])) for r in res["old_rows"]], dtype=np.int64)
notes.append(f"whole loop: {int((new_keys == old_keys).sum())} of {new_keys.size} rounded scores equal between the arms")
notes.append(f"whole loop, dict rows: {res['old_metrics']}")
notes.append(f"whole loop, matrix: {res['new_metrics']}")
cf = model._captured_forward
notes.append(f"whole loop, CapturedForward: {cf.stats}")

text = "\n".join(lines) + "\n\n" + "\n".join(f"- {s}" for s in notes) + "\n"
print(text, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
