"""ClipBertForPreTraining's labelled-rows mode (mlm_rows="labelled": select + gathered transform + LayerNorm + decoder + fused loss on the
labelled text rows only) against the CPU oracle, the untouched default mode, and the task-level consumers in clipbert_amd.tasks."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import parity_bounds
from clipbert_amd import optim, ops, tasks
from clipbert_amd import synthetic as S
from clipbert_amd.modeling import heads as H
from oracle import clipbert_oracle as O
from test_model_small import build, grads_of_oracle, make_batch, to_dev

NO_DROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
LOSS = lambda o: o["mlm_loss"].mean() + o["itm_loss"].mean()           # noqa: E731  (run_pretrain.py:387-395)
MLM_ONLY = ("cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias", "cls.predictions.transform.LayerNorm.weight",
            "cls.predictions.transform.LayerNorm.bias", "cls.predictions.bias")


def fp32_tols(hw):
    """the bounds of tests/test_model_small.py::test_forward_backward_matches_oracle_fp32"""
    ft = dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)
    return ft, (2e-3 if hw.name == "emul" else 5e-3)


def pretrain_batch(cfg, n_videos=2, lt=6, seed=5, labelled="alternate"):
    batch = make_batch(cfg, "pretraining", n_videos, 1, lt, seed)
    mlm = batch["text_input_ids"].clone()
    if labelled == "alternate":
        mlm[:, 1::2] = -100                                            # positions 0 ([CLS]), 2, 4, ... carry a label
    elif labelled == "none":
        mlm[:] = -100
    batch["mlm_labels"] = mlm
    batch["itm_labels"] = S.synthetic_labels(n_videos, 2, seed)
    return batch


def check_grads(hw, model, sdr, gt):
    """every parameter gradient against the oracle's autograd, relative to the tensor's max -- as test_model_small does it"""
    checked = 0
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g_ref = sdr[name].grad
        if g_ref is None:
            g_ref = torch.zeros_like(p, device="cpu")
        scale = max(g_ref.abs().max().item(), 1e-5)
        diff = p.grad.cpu() - g_ref
        err = diff.abs().max().item() / scale
        if hw.name == "emul":
            assert err < gt, f"{name}: relative grad error {err:.3e} (|g|max {scale:.3e})"
        else:                                                          # (a flipped ReLU / pool tie moves single elements: see test_model_small)
            l2 = diff.norm().item() / max(g_ref.norm().item(), 1e-5 * g_ref.numel() ** 0.5)
            assert l2 < gt, f"{name}: relative L2 grad error {l2:.3e} (|g| {g_ref.norm().item():.3e})"
            assert err < 10 * gt, f"{name}: worst-element grad error {err:.3e} (|g|max {scale:.3e})"
        checked += 1
    assert checked > 40, checked


def check_pred(out, ref, mlm):
    mask = mlm != -100
    pred = out["mlm_pred"].cpu()
    assert pred.shape == mlm.shape and pred.dtype == torch.int64
    assert torch.equal(pred[mask], ref["mlm_scores"].detach()[mask].argmax(-1)) and (pred[~mask] == -100).all()


@pytest.mark.parametrize("capacity,labelled", [(None, "alternate"), (64, "alternate"), (None, "none")])
def test_labelled_rows_match_oracle_fp32(hw, capacity, labelled):
    torch.manual_seed(0)
    cfg, sd, model = build("pretraining", {}, torch.float32, hw.dev)
    batch = pretrain_batch(cfg, labelled=labelled)
    ref, sdr = grads_of_oracle(sd, batch, cfg, "pretraining", LOSS)
    out = model(to_dev(dict(batch, mlm_rows="labelled", mlm_capacity=capacity), hw.dev))
    ft, gt = fp32_tols(hw)
    assert out["mlm_scores"] is None and set(out) == {"mlm_scores", "mlm_loss", "mlm_labels", "itm_scores", "itm_loss", "itm_labels", "mlm_pred"}
    assert out["mlm_loss"].shape == ref["mlm_loss"].shape and out["mlm_loss"].dtype == torch.float32
    torch.testing.assert_close(out["itm_scores"].cpu(), ref["itm_scores"], **ft)
    torch.testing.assert_close(out["mlm_loss"].cpu(), ref["mlm_loss"], **ft)
    check_pred(out, ref, batch["mlm_labels"])
    n_lab = int((batch["mlm_labels"] != -100).sum())
    assert model.transformer.mlm_counts.cpu().tolist() == [n_lab, 0]
    model.rt.bank.zero_grad()
    LOSS(out).backward()
    check_grads(hw, model, sdr, gt)
    if labelled == "none":                                             # zero, not NaN: the padding slots' lse is never used
        assert (out["mlm_loss"] == 0).all()
        params = dict(model.named_parameters())
        for name in MLM_ONLY:
            assert (params["transformer." + name].grad == 0).all(), name


def test_labelled_rows_with_pixel_random_sampling(hw):
    """train mode with pixel_random_sampling_size: L (hence the table's offsets, the row map and the dump row) follows the sampled length"""
    cfg, sd, model = build("pretraining", dict(NO_DROP, pixel_random_sampling_size=1), torch.float32, hw.dev)
    model.train()
    batch = pretrain_batch(cfg)
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k) for k, v in sd.items()}
    sdr["transformer.cls.predictions.decoder.weight"] = sdr["transformer.bert.embeddings.word_embeddings.weight"]
    sdr["transformer.cls.predictions.decoder.bias"] = sdr["transformer.cls.predictions.bias"]
    grid = O.grid_feat_backbone(sdr, batch["visual_inputs"], "cnn.")
    lv = grid.shape[2] * grid.shape[3]
    np.random.seed(7)
    idx = torch.from_numpy(np.sort(np.random.choice(lv, size=1, replace=False))).long()
    ref = O.pretraining_forward(sdr, batch["text_input_ids"], grid, batch["text_input_mask"], cfg, batch["mlm_labels"], batch["itm_labels"],
                                sample_idx=idx)
    LOSS(ref).backward()
    np.random.seed(7)                                                  # the product draws from the same global RNG
    model.rt.bank.zero_grad()
    out = model(to_dev(dict(batch, mlm_rows="labelled"), hw.dev))
    ft, gt = fp32_tols(hw)
    torch.testing.assert_close(out["itm_scores"].cpu(), ref["itm_scores"].detach(), **ft)
    torch.testing.assert_close(out["mlm_loss"].cpu(), ref["mlm_loss"].detach(), **ft)
    check_pred(out, ref, batch["mlm_labels"])
    LOSS(out).backward()
    check_grads(hw, model, sdr, gt)


def _parent_forward(tr, text_input_ids, visual_inputs, text_input_mask, mlm_labels=None, itm_labels=None, src_row=None):
    """ClipBertForPreTraining.forward as it stood before mlm_rows existed, launch for launch"""
    rt = tr.rt
    seq, pooled = tr.bert(text_input_ids, visual_inputs, text_input_mask, src_row)
    b, L, d = seq.shape
    lt = text_input_mask.shape[1]
    pred = tr.cls.predictions
    h = H._LinearFn.apply(rt.anchor, seq, rt, pred.transform.dense.weight, pred.transform.dense.bias, ops.ACT_GELU, False, (b, lt, L))
    h = H._LayerNormFn.apply(rt.anchor, h, rt, pred.transform.LayerNorm)
    scores = H._LinearFn.apply(rt.anchor, h, rt, pred.decoder.weight, pred.bias, ops.ACT_NONE, True, None)
    rel = tr.cls.seq_relationship
    itm = H._LinearFn.apply(rt.anchor, pooled, rt, rel.weight, rel.bias, ops.ACT_NONE, True, None)
    v = tr.config.vocab_size
    mlm_loss = H.cross_entropy_none(scores, mlm_labels.view(-1)) if mlm_labels is not None else 0
    itm_loss = H.cross_entropy_none(itm.view(-1, 2), itm_labels.view(-1)) if itm_labels is not None else 0
    return dict(mlm_scores=scores.view(b, lt, v), mlm_loss=mlm_loss, mlm_labels=mlm_labels, itm_scores=itm, itm_loss=itm_loss, itm_labels=itm_labels)


def test_default_mode_is_untouched(hw):
    """mlm_rows omitted == mlm_rows="all" == the forward that never heard of the argument: the outputs and every gradient bit for bit --
    except the embedding tables, whose gradients the embedding backward adds up through fp32 atomics in whatever order the workgroups
    arrive (two runs of the SAME code differ there in the last bit): those are held to the bound tests/test_model_small.py puts on one
    gradient buffer computed twice (rtol 1e-5, atol 1e-7)."""
    cfg, sd, model = build("pretraining", {}, torch.float32, hw.dev)
    batch = pretrain_batch(cfg)
    bank = model.rt.bank
    with torch.no_grad():                                              # the CNN once: its gradients are a function of d(grid), compared below
        grid0 = model.grid_features(batch["visual_inputs"].to(hw.dev))

    def run(extra, forward=None):
        grid = grid0.clone().requires_grad_(True)
        b = to_dev(dict(batch, **extra), hw.dev)
        b["visual_inputs"] = grid
        bank.zero_grad()
        if forward is None:
            out = model.forward_from_grid(b)
        else:
            del b["n_examples_list"]
            out = forward(model.transformer, **b)
        LOSS(out).backward()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.requires_grad and not n.startswith("cnn.")}
        return out, dict(grads, grid=grid.grad.clone())

    base, g_base = run({}, forward=_parent_forward)
    for extra in ({}, dict(mlm_rows="all"), dict(mlm_rows="all", mlm_capacity=64)):
        out, g = run(extra)
        assert set(out) == set(base) and "mlm_pred" not in out
        for k in ("mlm_scores", "mlm_loss", "itm_scores", "itm_loss"):
            assert torch.equal(out[k], base[k]), k
        exact = 0
        for name in g_base:
            if "embeddings" in name:
                torch.testing.assert_close(g[name], g_base[name], rtol=1e-5, atol=1e-7)
            else:
                assert torch.equal(g[name], g_base[name]), name
                exact += 1
        assert exact > 30 and all(("transformer." + n) in g_base for n in MLM_ONLY)
    assert max(t.abs().max().item() for t in g_base.values()) > 0
    with pytest.raises(ValueError):
        model(to_dev(dict(batch, mlm_labels=None, mlm_rows="labelled"), hw.dev))
    with pytest.raises(ValueError):
        model(to_dev(dict(batch, mlm_rows="some"), hw.dev))


def test_bf16_labelled_no_worse_than_all(hw):
    """Both modes in bf16 against the fp32 oracle on one batch: the labelled-rows error of mlm_loss and of each gradient is held to
    parity_bounds.FACTOR x the "all"-mode error of the same quantity (floored at the fp32 tolerance); mlm_pred equals the "all"-mode
    arg-max wherever the oracle's top-1 / top-2 margin exceeds 10 x the measured logit error."""
    cfg, sd, model = build("pretraining", {}, torch.bfloat16, hw.dev, seed=8)
    batch = pretrain_batch(cfg, seed=29)                               # (seeds whose oracle margins decide five of the six positions by > 0.16)
    ref, sdr = grads_of_oracle(sd, batch, cfg, "pretraining", LOSS)
    bank = model.rt.bank
    ft, gt = fp32_tols(hw)
    res = {}
    for mode in ("all", "labelled"):
        bank.zero_grad()
        out = model(to_dev(dict(batch, mlm_rows=mode), hw.dev))
        LOSS(out).backward()
        res[mode] = (out, {n: p.grad.float().cpu().clone() for n, p in model.named_parameters() if p.requires_grad})
    loss_ref = ref["mlm_loss"].detach()
    err = {m: (res[m][0]["mlm_loss"].cpu() - loss_ref).abs().max().item() for m in res}
    floor = ft["atol"] + ft["rtol"] * loss_ref.abs().max().item()
    print(f"\n[{hw.name}] bf16 mlm_loss error: all {err['all']:.3e}, labelled {err['labelled']:.3e}")
    assert err["labelled"] <= max(parity_bounds.FACTOR * err["all"], floor)
    worst = (0.0, "")
    for name, g_all in res["all"][1].items():
        g_ref = sdr[name].grad if sdr[name].grad is not None else torch.zeros_like(g_all)
        scale = max(g_ref.abs().max().item(), 1e-5)
        e_all = (g_all - g_ref).abs().max().item() / scale
        e_lab = (res["labelled"][1][name] - g_ref).abs().max().item() / scale
        worst = max(worst, (e_lab / max(e_all, 1e-12), name))
        assert e_lab <= max(parity_bounds.FACTOR * e_all, gt), f"{name}: labelled {e_lab:.3e} vs all {e_all:.3e}"
    print(f"[{hw.name}] worst labelled / all gradient error ratio: {worst[0]:.3f} ({worst[1]})")
    mlm = batch["mlm_labels"]
    mask = mlm != -100
    scores_all = res["all"][0]["mlm_scores"].float().cpu()
    logit_err = (scores_all - ref["mlm_scores"].detach()).abs().max().item()
    top2 = ref["mlm_scores"].detach().topk(2, dim=-1).values
    decided = mask & ((top2[..., 0] - top2[..., 1]) > 10 * logit_err)
    assert decided.sum().item() >= 0.75 * mask.sum().item(), (decided.sum().item(), mask.sum().item(), logit_err)
    pred = res["labelled"][0]["mlm_pred"].cpu()
    assert torch.equal(pred[decided], scores_all.argmax(-1)[decided]) and (pred[~mask] == -100).all()


# ---- task level --------------------------------------------------------------------------------------------------------------------

def _tcfg(**kw):
    return SimpleNamespace(**dict(dict(use_mlm=True, use_itm=True, mlm_capacity=None, learning_rate=1e-3, cnn_learning_rate=1e-3, decay="linear",
                                       cnn_lr_decay="constant", num_train_steps=10, warmup_ratio=0.0, num_frm=2, train_n_clips=1,
                                       score_agg_func="mean"), **kw))


def test_fixed_capacity_overflow_raises_in_validation(hw):
    cfg, sd, model = build("pretraining", dict(max_position_embeddings=80), torch.float32, hw.dev)
    batch = make_batch(cfg, "pretraining", 2, 1, 40)
    batch["mlm_labels"] = batch["text_input_ids"].clone()              # 80 labelled rows
    batch["itm_labels"] = S.synthetic_labels(2, 2, 5)
    loader = [to_dev(batch, hw.dev)]
    with pytest.raises(RuntimeError, match="dropped 16"):
        tasks.validate_pretrain(model, loader, _tcfg(mlm_rows="labelled", mlm_capacity=64))
    assert model.transformer.mlm_counts.cpu().tolist() == [80, 16]
    model.transformer.mlm_counts = None
    log = tasks.validate_pretrain(model, loader, _tcfg(mlm_rows="labelled", mlm_capacity=80))          # (80 -> 128 slots)
    assert log["valid/mlm_loss"] > 0 and model.transformer.mlm_counts.cpu().tolist() == [80, 0]


class _GridCache(torch.nn.Module):
    """the model with each batch's grid features computed once: the task functions under test call it many times on the same frames"""
    def __init__(self, model):
        super().__init__()
        self.model, self.grids = model, {}

    transformer = property(lambda self: self.model.transformer)

    def forward(self, batch):
        vis = batch["visual_inputs"]
        if vis.data_ptr() not in self.grids:
            with torch.no_grad():
                self.grids[vis.data_ptr()] = self.model.grid_features(vis)
        return self.model.forward_from_grid(dict(batch, visual_inputs=self.grids[vis.data_ptr()]))


def test_pretrain_loss_and_validation(hw):
    cfg, sd, model = build("pretraining", {}, torch.float32, hw.dev)
    model = _GridCache(model).eval()
    batches = [pretrain_batch(cfg, seed=s) for s in (5, 6, 7)]
    with torch.no_grad():
        refs = [O.clipbert_forward(sd, dict(b, n_examples_list=[1, 1]), cfg, "pretraining") for b in batches]
    loader = [to_dev(b, hw.dev) for b in batches]
    # pretrain_loss honours use_mlm / use_itm (run_pretrain.py:196-202, 387-395), in both modes
    mlm, itm = refs[0]["mlm_loss"].mean(), refs[0]["itm_loss"].mean()
    with torch.no_grad():
        for rows in ("labelled", "all"):
            for use_mlm, use_itm, want in ((True, True, mlm + itm), (True, False, mlm), (False, True, itm)):
                got = tasks.pretrain_loss(model, dict(loader[0]), _tcfg(mlm_rows=rows, use_mlm=use_mlm, use_itm=use_itm))
                torch.testing.assert_close(got.cpu(), want, rtol=2e-3, atol=2e-4)
        assert torch.equal(tasks.pretrain_loss(model, dict(loader[0]), _tcfg()), tasks.pretrain_loss(model, dict(loader[0]), _tcfg(mlm_rows="labelled")))
    # validate_pretrain: the reference's expression (run_pretrain.py:229-266) on the oracle's outputs
    n_tok = sum(int((b["mlm_labels"] != -100).sum()) for b in batches)
    n_ok = sum(int((r["mlm_scores"][b["mlm_labels"] != -100].max(dim=-1)[1] == b["mlm_labels"][b["mlm_labels"] != -100]).sum()) for b, r in zip(batches, refs))
    i_ok = sum(int((r["itm_scores"].max(dim=-1)[1] == b["itm_labels"]).sum()) for b, r in zip(batches, refs))
    want = {"valid/mlm_loss": sum(float(r["mlm_loss"].sum()) for r in refs) / n_tok, "valid/mlm_acc": n_ok / n_tok,
            "valid/itm_loss": sum(float(r["itm_loss"].sum()) for r in refs) / 6, "valid/itm_acc": i_ok / 6}
    logs = {rows: tasks.validate_pretrain(model, loader, _tcfg(mlm_rows=rows)) for rows in ("labelled", "all")}
    for rows, log in logs.items():
        assert set(log) == set(want)
        for k in want:
            assert log[k] == pytest.approx(want[k], rel=2e-3, abs=2e-4), (rows, k)
    for k in want:
        assert logs["labelled"][k] == pytest.approx(logs["all"][k], rel=1e-5, abs=1e-6), k
    assert logs["labelled"]["valid/mlm_acc"] == logs["all"]["valid/mlm_acc"]


def test_train_step_loss_fn(hw):
    """train_step(loss_fn=tasks.pretrain_loss) drives the pretraining head and the optimizer moves the TIED word-embedding weight;
    without loss_fn the step is what it was: two runs of an existing retrieval case, one naming loss_fn=None, end bit-equal (embedding tables: see test_default_mode_is_untouched)"""
    cfg, sd, model = build("pretraining", NO_DROP, torch.float32, hw.dev)
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
    batch = to_dev(pretrain_batch(cfg), hw.dev)
    word = dict(model.named_parameters())["transformer.bert.embeddings.word_embeddings.weight"]
    before = word.detach().float().cpu().clone()
    with torch.no_grad():
        want = tasks.pretrain_loss(model, dict(batch), _tcfg())
    loss = tasks.train_step(model, opt, dict(batch), _tcfg(), global_step=0, loss_fn=tasks.pretrain_loss)
    assert torch.isfinite(loss).all() and torch.equal(loss, want)
    moved = (word.detach().float().cpu() - before).abs().amax(1)
    labelled_ids = batch["mlm_labels"][batch["mlm_labels"] != -100].unique().cpu()
    assert (moved[labelled_ids] > 0).all()
    ends = []
    for kw in ({}, dict(loss_fn=None)):
        rcfg, rsd, ret = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), torch.float32, hw.dev)
        ret.eval()
        ropt = optim.FusedAdamW(ret.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=-1.0)
        rb = make_batch(rcfg, "retrieval", 1, 2, 6)
        rb["labels"] = S.synthetic_labels(2, 2, 5)
        rloss = tasks.train_step(ret, ropt, to_dev(rb, hw.dev), _tcfg(), global_step=0, **kw)
        ends.append((rloss.cpu(), {n: (p.grad.cpu().clone(), p.detach().cpu().clone()) for n, p in ret.named_parameters() if p.requires_grad}))
    assert torch.equal(ends[0][0], ends[1][0])
    for name, (g0, w0) in ends[0][1].items():                          # (no norm clipping above: the clip coefficient would tie every weight to
        g1, w1 = ends[1][1][name]                                      #  the embedding gradients, whose atomic sums differ run to run)
        if "embeddings" in name:
            torch.testing.assert_close(g1, g0, rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(w1, w0, rtol=1e-5, atol=1e-7)
        else:
            assert torch.equal(g1, g0) and torch.equal(w1, w0), name
