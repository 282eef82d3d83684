"""The pretraining head ALONE, forward + backward from a fixed (32, 130, 768) encoder output in bf16 (the shipped pretraining shape:
train_batch_size 32, max_txt_len 30 -> 960 text rows, pixel_random_sampling_size 100 -> L = 130), ~10 % of the text rows labelled by a
seeded mask: mlm_rows = "all" (every text row through transform, LayerNorm, decoder and cb_cross_entropy) against "labelled" with
mlm_capacity None (960 slots) and 256.  Each mode is one hipGraph of forward + backward; the three are replayed alternately, 5 rounds of
50 replays each between HIP events after 20 warm-up replays, best round reported with the spread.  Writes profiles/mlm_head_probe.json.

    python tools/mlm_head_probe.py [--out profiles/mlm_head_probe.json]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from clipbert_amd import clips, ops
from clipbert_amd import modeling as M
from clipbert_amd import synthetic as S
from clipbert_amd.bench.step import BASE_CONFIG
from clipbert_amd.modeling import heads as H

B, LT, L, SEED = 32, 30, 130, 11


def all_rows_head(tr, seq, lt, labels):
    """the head stages of ClipBertForPreTraining.forward(mlm_rows="all")"""
    rt, pred = tr.rt, tr.cls.predictions
    b, l, _ = seq.shape
    h = H._LinearFn.apply(rt.anchor, seq, rt, pred.transform.dense.weight, pred.transform.dense.bias, ops.ACT_GELU, False, (b, lt, l))
    h = H._LayerNormFn.apply(rt.anchor, h, rt, pred.transform.LayerNorm)
    scores = H._LinearFn.apply(rt.anchor, h, rt, pred.decoder.weight, pred.bias, ops.ACT_NONE, True, None)
    return H.cross_entropy_none(scores, labels.view(-1))


def logits_bytes(rows, v):
    """fp32 scores + what the backward allocates next to them"""
    return dict(all=rows * ((v + 3) // 4 * 4) * 4 * 2 + rows * v * 2,                  # scores, fp32 gradient, its bf16 cast
                labelled=lambda cap: cap * ((v + 3) // 4 * 4) * 4 + cap * ((v + 7) // 8 * 8) * 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mlm_head_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mlm_head_probe: needs the GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda", 0)
    cfg = dict(BASE_CONFIG, attention_probs_dropout_prob=0.0, hidden_dropout_prob=0.0)
    model = M.ClipBert(cfg, detectron2_model_cfg="R-50-grid.yaml", transformer_cls=M.ClipBertForPreTraining)
    model.load_state_dict(S.full_state_dict(cfg, "pretraining", SEED), strict=True)
    model.to(dev).train()
    model.prepare(dtype=torch.bfloat16, device=dev)
    tr, bank = model.transformer, model.rt.bank
    v, d = cfg["vocab_size"], cfg["hidden_size"]
    g = torch.Generator().manual_seed(SEED)
    seq = torch.randn(B, L, d, generator=g).to(dev).bfloat16().requires_grad_(True)
    ids = torch.randint(1000, v, (B, LT), generator=g)
    labels = torch.where(torch.rand(B, LT, generator=g) < 0.10, ids, torch.full_like(ids, -100)).to(dev)
    n_lab = int((labels != -100).sum())
    modes = {"all": lambda: all_rows_head(tr, seq, LT, labels),
             "labelled": lambda: tr.labelled_mlm_head(seq, LT, labels, None)[0],
             "labelled_cap256": lambda: tr.labelled_mlm_head(seq, LT, labels, 256)[0]}

    def step(fn):
        seq.grad = None
        loss = clips.mean_loss(fn())
        loss.backward()
        return loss

    graphs, check = {}, {}
    side = torch.cuda.Stream(device=dev)
    for name, fn in modes.items():
        bank.zero_grad()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(2):
                step(fn)
            bank.zero_grad()
            loss = step(fn)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        check[name] = (float(loss.detach()), seq.grad.float().clone(), bank.grad.clone())
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step(fn)
        graphs[name] = gr
    # faster and different is not faster: the three modes agree on the loss and on every gradient they produce
    ref = check["all"]
    agree = {}
    for name, (loss, dseq, grad) in check.items():
        agree[name] = dict(loss=loss, dseq_rel_l2=float((dseq - ref[1]).norm() / ref[1].norm()), grad_rel_l2=float((grad - ref[2]).norm() / ref[2].norm()))
    for gr in graphs.values():
        for _ in range(20):
            gr.replay()
    torch.cuda.synchronize()
    rounds = {name: [] for name in graphs}
    for _ in range(5):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            rounds[name].append(e0.elapsed_time(e1) / 50 * 1e3)
    nbytes = logits_bytes(B * LT, v)
    alloc = {"all": nbytes["all"], "labelled": nbytes["labelled"](960), "labelled_cap256": nbytes["labelled"](256)}
    out = dict(shape=dict(B=B, Lt=LT, L=L, d=d, V=v, labelled_rows=n_lab), dtype="bf16", device=torch.cuda.get_device_name(0),
               method="hipGraph of head forward + backward per mode; 20 warm-up replays; 5 alternating rounds x 50 replays between HIP events",
               modes={name: dict(us_best=min(r), us_worst=max(r), us_rounds=r, logits_bytes=alloc[name], **agree[name]) for name, r in rounds.items()},
               dropped=int(tr.mlm_counts[1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    for name, m in out["modes"].items():
        print(f"{name:16s} {m['us_best']:9.1f} us (worst round {m['us_worst']:9.1f})  logits {m['logits_bytes'] / 1e6:7.1f} MB  loss {m['loss']:.5f}  "
              f"dseq rel l2 {m['dseq_rel_l2']:.2e}  grad rel l2 {m['grad_rel_l2']:.2e}", flush=True)


if __name__ == "__main__":
    main()
