"""The image-VQA task through the product Python layer: ClipBertForSequenceClassification on SPARSE answers (the fused last-Linear +
BCE node) against the CPU oracle on the dense targets and against the product's own dense ``labels`` path, tasks.vqa_loss through
start_training with and without captured steps, and tasks.validate_vqa against a restatement from the logits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clipbert_amd import captured as CAP
from clipbert_amd import optim, tasks
from clipbert_amd import synthetic as S
from clipbert_amd.data import vqa_dense_targets
from oracle import clipbert_oracle as O
from test_captured_loop import NO_DROP, _tcfg
from test_model_small import assert_grads_match_oracle, build, forward_tol, grads_of_oracle, make_batch, to_dev

HEAD = "sequence_classification"
SCORES = (0.3, 0.6, 0.9, 1.0)


def _tables(n_labels, counts, seed, k=10):
    """(ids int32, scores fp32) (len(counts), k): question i has counts[i] distinct answers"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((len(counts), k), -1, dtype=torch.int32)
    scores = torch.zeros(len(counts), k)
    for i, n in enumerate(counts):
        ids[i, :n] = torch.randperm(n_labels, generator=g)[:n].to(torch.int32)
        scores[i, :n] = torch.tensor(SCORES)[torch.randint(0, 4, (n,), generator=g)]
    return ids, scores


def _grads(model):
    return {name: p.grad.detach().cpu().clone() for name, p in model.named_parameters() if p.requires_grad}


@pytest.mark.parametrize("n_labels", [6, 3129])
def test_sparse_answers_match_oracle_and_the_dense_path_fp32(hw, n_labels):
    """2 videos x 2 questions with 0 / 1 / 3 / 5 answers: logits, row-sum loss, arg-max and every parameter gradient of loss.mean()
    against the oracle on the dense targets (tolerances of tests/test_model_small.py), then the same gradients against the product's
    own dense ``labels`` path (loss.sum(1).mean()) within the same bounds"""
    cfg, sd, model = build(HEAD, dict(num_labels=n_labels, loss_type="bce"), torch.float32, hw.dev)
    batch = make_batch(cfg, HEAD, 2, 2, 6)
    ids, scores = _tables(n_labels, [0, 1, 3, 5], seed=n_labels)
    dense = vqa_dense_targets(ids, scores, n_labels)
    ref, sdr = grads_of_oracle(sd, dict(batch, labels=dense), cfg, HEAD, lambda o: o["loss"].sum(1).mean())
    model.rt.bank.zero_grad()
    out = model(to_dev(dict(batch, answer_ids=ids, answer_scores=scores), hw.dev))
    ft = forward_tol(hw)
    assert out["loss"].shape == (4,) and out["pred"].dtype == torch.int64 and out["pred_score"].dtype == torch.float32
    torch.testing.assert_close(out["logits"].cpu(), ref["logits"].detach(), **ft)
    torch.testing.assert_close(out["loss"].cpu(), ref["loss"].detach().sum(1), **ft)
    assert torch.equal(out["pred"].cpu(), ref["logits"].argmax(1))
    assert torch.equal(out["pred_score"].cpu(), dense[torch.arange(4), out["pred"].cpu()])
    out["loss"].mean().backward()
    assert_grads_match_oracle(hw, model, sdr)
    sparse = _grads(model)

    model.rt.bank.zero_grad()
    out_d = model(to_dev(dict(batch, labels=dense), hw.dev))
    assert out_d["loss"].shape == (4, n_labels) and "pred" not in out_d                    # the dense path is what it was
    torch.testing.assert_close(out_d["loss"].sum(1).cpu(), out["loss"].cpu(), **ft)
    out_d["loss"].sum(1).mean().backward()
    gt = 2e-3 if hw.name == "emul" else 5e-3
    for name, g_d in _grads(model).items():
        diff = sparse[name] - g_d
        scale = max(g_d.abs().max().item(), 1e-5)
        l2 = diff.norm().item() / max(g_d.norm().item(), 1e-5 * g_d.numel() ** 0.5)
        assert (diff.abs().max().item() / scale < gt) if hw.name == "emul" else (l2 < gt and diff.abs().max().item() / scale < 10 * gt), name


def test_sparse_answers_bf16_within_the_bf16_mode_bound(hw):
    """No new tolerance: test_bf16_mode_close (tests/test_model_small.py) holds bf16 logits and per-example losses to 5e-2 of the fp32
    oracle; here the logits and the ROW SUM of the six losses are held to that.  The dense bf16 path on the same batch (the parent: only
    the order of the additions in the two backward GEMMs differs, the forward GEMM is the same launch) is printed next to it.  Measured
    max |error| (logits / row-sum loss), sparse vs dense:
      host emulator  logits 1.187e-04 vs 1.187e-04    loss 7.391e-05 vs 7.391e-05
      MI355X         logits 9.879e-05 vs 9.879e-05    loss 6.676e-05 vs 6.628e-05"""
    n_labels = 6
    cfg, sd, model = build(HEAD, dict(num_labels=n_labels, loss_type="bce"), torch.bfloat16, hw.dev)
    batch = make_batch(cfg, HEAD, 1, 2, 5)
    ids, scores = _tables(n_labels, [2, 4], seed=9)
    dense = vqa_dense_targets(ids, scores, n_labels)
    with torch.no_grad():
        ref = O.clipbert_forward(sd, dict(batch, labels=dense), cfg, HEAD)
        out = model(to_dev(dict(batch, answer_ids=ids, answer_scores=scores), hw.dev))
        out_d = model(to_dev(dict(batch, labels=dense), hw.dev))
    want = ref["loss"].sum(1)
    e_logits, e_loss = (out["logits"].cpu() - ref["logits"]).abs().max().item(), (out["loss"].cpu() - want).abs().max().item()
    d_logits, d_loss = (out_d["logits"].cpu() - ref["logits"]).abs().max().item(), (out_d["loss"].sum(1).cpu() - want).abs().max().item()
    print(f"\n[{hw.name}] bf16 max |error| vs the fp32 oracle: logits {e_logits:.3e} (dense path {d_logits:.3e}), row-sum loss {e_loss:.3e} (dense path {d_loss:.3e})")
    assert e_logits < 5e-2 and e_loss < 5e-2
    assert torch.equal(out["pred"].cpu(), out["logits"].cpu().argmax(1))


def test_argument_errors(hw, monkeypatch):
    """raised by the head before anything runs: sparse answers with dense labels, one table without the other, loss_type "ce", num_labels 1"""
    n_labels = 6
    cfg, _sd, model = build(HEAD, dict(num_labels=n_labels, loss_type="bce"), torch.float32, hw.dev)
    batch = make_batch(cfg, HEAD, 1, 2, 5)
    ids, scores = _tables(n_labels, [2, 4], seed=9)
    head = model.transformer
    args = to_dev(dict(text_input_ids=batch["text_input_ids"], visual_inputs=torch.zeros(1, 1, 2, 4, cfg["hidden_size"]),
                       text_input_mask=batch["text_input_mask"], answer_ids=ids, answer_scores=scores), hw.dev)
    with pytest.raises(ValueError, match="exclude"):
        head(**args, labels=hw(vqa_dense_targets(ids, scores, n_labels)))
    with pytest.raises(ValueError, match="come together"):
        head(**dict(args, answer_scores=None))
    monkeypatch.setattr(head.config, "loss_type", "ce")
    with pytest.raises(ValueError, match="loss_type 'bce'"):
        head(**args)
    monkeypatch.setattr(head.config, "loss_type", "bce")
    monkeypatch.setattr(head.config, "num_labels", 1)
    with pytest.raises(ValueError, match="num_labels > 1"):
        head(**args)


def _vqa_batch(frames, n_labels, counts, seed, vocab, dev, lt=6):
    ids, mask = S.synthetic_text(len(counts), lt, seed, vocab)
    a_ids, a_scores = _tables(n_labels, counts, seed)
    b = dict(visual_inputs=frames, text_input_ids=ids.clamp(max=vocab - 1), text_input_mask=mask, answer_ids=a_ids, answer_scores=a_scores,
             n_examples_list=[len(counts)], question_ids=[100 * seed + i for i in range(len(counts))],
             answer_types=[tasks.VQA_ANSWER_TYPES[(seed + i) % 3] for i in range(len(counts))])
    return to_dev(b, dev)


def test_start_training_with_vqa_loss_captured_reaches_the_same_parameters(hw):
    """four optimizer steps over a loader of two batches of ONE signature -- equal shapes, 1 / 4 and 3 / 0 answers per question: captured
    (dry on the emulator, hipGraphs on the GPU) against capture=False; the answer tables are ordinary static buffers of the one graph"""
    n_labels = 6
    finals, steppers = [], []
    for capture in (False, "dry" if hw.name == "emul" else True):
        cfg, _sd, model = build(HEAD, dict(num_labels=n_labels, loss_type="bce", **NO_DROP), torch.float32 if hw.name == "emul" else torch.bfloat16, hw.dev)
        model.train(True)
        opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
        tcfg = _tcfg(train_n_clips=1, num_frm=1, num_labels=n_labels, num_train_steps=4, warmup_ratio=0.5, train_batch_size=1, valid_steps=0)
        one_image = lambda seed: S.synthetic_frames(1, 1, 64, seed).contiguous()      # noqa: E731
        loader = [_vqa_batch(one_image(41), n_labels, [1, 4], 41, cfg["vocab_size"], hw.dev), _vqa_batch(one_image(42), n_labels, [3, 0], 42, cfg["vocab_size"], hw.dev)]
        if capture:
            capture = CAP.CapturedStep(model, opt, tcfg, loss_fn=tasks.vqa_loss, mode="dry" if capture == "dry" else "graph")
            steppers.append(capture)
        assert tasks.start_training(model, opt, loader, tcfg, loss_fn=tasks.vqa_loss, capture=capture) == 4 and opt.step_count == 4
        finals.append(model.rt.bank.master.clone())
    st = steppers[0]
    assert st.log == ["eager"] * 2 + ["replay"] * 2 and st.stats["captures"] == 1 and st.stats["fallbacks"] == 0 and st.stats["replays"] == 2, (st.log, st.stats)
    assert set(st.graphs[next(iter(st.graphs))].bufs) == {"visual_inputs", "text_input_ids", "text_input_mask", "answer_ids", "answer_scores"}
    assert float((finals[0] - finals[1]).abs().max()) <= 1e-6 * float(finals[0].abs().max())


def test_validate_vqa_against_a_restatement_from_the_logits(hw):
    n_labels = 6
    cfg, _sd, model = build(HEAD, dict(num_labels=n_labels, loss_type="bce"), torch.float32, hw.dev)
    model.train(True)
    frames = [S.synthetic_frames(1, 1, 64, 50 + i).contiguous() for i in range(2)]
    batches = [_vqa_batch(frames[i], n_labels, [1, 1], 50 + i, cfg["vocab_size"], hw.dev) for i in range(2)]
    plain = lambda b: {k: v for k, v in b.items() if k not in ("answer_ids", "answer_scores", "answer_types")}      # noqa: E731
    # the restatement's inputs: eval-mode logits of the questions, and answer tables built around their arg-max -- question 0 of each batch
    # has its prediction among its answers (score 0.6 / 0.9), question 1 has not
    model.eval()
    with torch.no_grad():
        logits = [model({k: v for k, v in plain(b).items() if k != "question_ids"})["logits"].cpu().double() for b in batches]
    model.train(True)
    label2ans = {i: f"answer {i}" for i in range(n_labels)}
    for i, b in enumerate(batches):
        pred = logits[i].argmax(1).tolist()
        ids = torch.full((2, 10), -1, dtype=torch.int32)
        sc = torch.zeros(2, 10)
        ids[0, :2], sc[0, :2] = torch.tensor([(pred[0] + 1) % n_labels, pred[0]], dtype=torch.int32), torch.tensor([0.3, (0.6, 0.9)[i]])
        ids[1, :1], sc[1, :1] = (pred[1] + 2) % n_labels, 1.0
        b["answer_ids"], b["answer_scores"] = ids.to(hw.dev), sc.to(hw.dev)
        b["answer_types"] = ["yes/no", "other"] if i == 0 else ["number", "other"]
    dense = [vqa_dense_targets(b["answer_ids"], b["answer_scores"], n_labels).double() for b in batches]
    want_loss = sum(float(F.binary_cross_entropy_with_logits(lg, t, reduction="sum")) for lg, t in zip(logits, dense)) / 4
    want_rows = [dict(question_id=q, answer=label2ans[p]) for b, lg in zip(batches, logits) for q, p in zip(b["question_ids"], lg.argmax(1).tolist())]
    want = {"valid/overall_acc": round(100 * (np.float64(np.float32(0.6)) + np.float64(np.float32(0.9))) / 4, 2),
            "valid/yes/no_acc": round(100 * float(np.float32(0.6)), 2), "valid/number_acc": round(100 * float(np.float32(0.9)), 2), "valid/other_acc": 0.0}

    rows, log = tasks.validate_vqa(model, batches, cfg, label2ans=label2ans)
    assert model.training                                                                  # the training flag is restored
    assert rows == want_rows
    assert log.pop("valid/loss") == pytest.approx(want_loss, rel=1e-5)
    assert log == want, (log, want)
    # without answer_types: the overall accuracy only; without label2ans: the ids
    rows, log = tasks.validate_vqa(model, [{k: v for k, v in b.items() if k != "answer_types"} for b in batches], cfg)
    assert [r["answer"] for r in rows] == [p for lg in logits for p in lg.argmax(1).tolist()]
    assert set(log) == {"valid/loss", "valid/overall_acc"} and log["valid/overall_acc"] == want["valid/overall_acc"]
    # a test set: no answers, rows from logits.max(dim=-1)[1], no scores
    model.eval()
    rows, log = tasks.validate_vqa(model, [dict(plain(b), labels=None) for b in batches], cfg, label2ans=label2ans)
    assert rows == want_rows and log == {"valid/loss": 0.0} and not model.training
