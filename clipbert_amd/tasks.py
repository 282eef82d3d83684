"""Task-loop pieces around the hot path: the training step and the retrieval inference of
src/tasks/run_video_retrieval.py, and its metrics, on top of clipbert_amd.modeling.  Host logic only -- every tensor op is
a libclipbert_hip kernel reached through the model / clips / optimizer objects.

``cfg`` is any object with the reference's config attributes (src/configs/*.json): num_frm, train_n_clips,
inference_n_clips, score_agg_func, inference_batch_size, learning_rate, decay, cnn_learning_rate, cnn_lr_decay,
num_train_steps, warmup_ratio, step_decay_epochs, cnn_step_decay_epochs, transformer_lr_mul, cnn_lr_mul."""
import math
from collections import defaultdict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import clips, ops
from .optim import get_lr_sched


def _get(cfg, name, default=None):
    return cfg.get(name, default) if isinstance(cfg, dict) else getattr(cfg, name, default)


# ---- training (run_video_retrieval.py:380-494) ------------------------------------------------------------------------
_SKIP_KEYS = ("visual_inputs", "caption_ids", "vid_id", "question_ids", "n_examples_list", "answer_types")


def _pair_counts(cfg, n_examples_list):
    """forward_step of run_video_qa.py:206-210: the multiple-choice tasks present every (question, option) pair as its own
    text row, so each video's count is multiplied by cfg.num_labels before the model call."""
    counts = list(n_examples_list)
    if cfg is not None and _get(cfg, "task") in ("action", "transition"):
        nl = int(_get(cfg, "num_labels"))
        counts = [e * nl for e in counts]
    return counts


def forward_clips_stack(model, batch: Dict, num_clips: int, num_frm: int, fold: bool = True, cfg=None,
                        with_labels: bool = False) -> torch.Tensor:
    """The clip loop of the reference's training / validation steps (run_video_retrieval.py:391-401, run_video_qa.py:
    470-482): (B, num_clips*num_frm, 3, H, W) frames -> the (num_clips, B', C) stack of per-clip logits.

    fold=True (default) runs ALL clips as one forward: the frame tensor is viewed as (B*num_clips, num_frm, ...) -- no
    copy -- for one CNN batch, the text rows are repeated clip-major for one encoder batch of num_clips*B' pairs
    (ClipBert.forward_from_grid(clip_fold=...)).  The reference pools at logit level, so this is results-identical to its
    loop while every GEMM sees num_clips x the rows.  fold=False keeps the loop (one forward per clip)."""
    vis = batch["visual_inputs"]
    bsz = vis.shape[0]
    counts = _pair_counts(cfg, batch["n_examples_list"])
    labels = batch.get("labels") if with_labels else None
    extra = {k: v for k, v in batch.items() if k not in _SKIP_KEYS + ("labels", "text_input_ids", "text_input_mask")}
    ids, mask = batch["text_input_ids"], batch["text_input_mask"]
    if fold and num_clips > 1:
        grid = model.grid_features(vis.view(bsz * num_clips, num_frm, *vis.shape[2:]))
        # (the text rows are NOT repeated: forward_from_grid(clip_fold=n) lets every clip read the one caption batch in place)
        mini = dict(extra, visual_inputs=grid, text_input_ids=ids, text_input_mask=mask, labels=None, n_examples_list=counts)
        lg = model.forward_from_grid(mini, clip_fold=num_clips)["logits"]
        return lg.reshape(num_clips, lg.shape[0] // num_clips, *lg.shape[1:])
    vis = vis.view(bsz, num_clips, num_frm, *vis.shape[2:])
    logits = []
    for c in range(num_clips):
        mini = dict(extra, visual_inputs=vis[:, c].contiguous() if num_clips > 1 else vis[:, 0], text_input_ids=ids,
                    text_input_mask=mask, labels=labels, n_examples_list=list(counts))
        logits.append(model(mini)["logits"])
    return torch.stack(logits)


def forward_clips(model, batch: Dict, num_clips: int, num_frm: int, fold: bool = True, cfg=None) -> List[torch.Tensor]:
    """forward_clips_stack as the list of per-clip logits the reference's loop builds."""
    return list(forward_clips_stack(model, batch, num_clips, num_frm, fold=fold, cfg=cfg).unbind(0))


def training_loss(model, logits, labels, n_examples_list, pool_method: str) -> torch.Tensor:
    """:402-419: pool the clips (``logits``: list of per-clip logits or their (n_clips, B', C) stack) and take the mean
    per-pair loss."""
    if pool_method == "lse":
        return clips.mean_loss(clips.lse_stack_train_loss(logits, labels))
    pooled = clips.aggregate_clip_logits(logits, pool_method)
    if getattr(model, "retrieval", False):
        _, loss = model.transformer.calc_loss(pooled, labels, sample_size=len(n_examples_list))
    else:                                                   # QA heads (run_video_qa.py:417-419)
        _, loss = model.transformer.calc_loss(pooled, labels)
    return clips.mean_loss(loss)


def set_learning_rates(optimizer, cfg, global_step: int, n_epoch: int = 0):
    """:438-467: transformer / CNN schedules onto the 8 parameter groups (0,1 new transformer; 2,3 transformer; 4,5 new
    CNN; 6,7 CNN)."""
    lr_t = get_lr_sched(global_step, _get(cfg, "decay", "linear"), _get(cfg, "learning_rate"), _get(cfg, "num_train_steps"),
                        warmup_ratio=_get(cfg, "warmup_ratio", 0.1), decay_epochs=_get(cfg, "step_decay_epochs", ()),
                        multi_step_epoch=n_epoch)
    lr_c = get_lr_sched(global_step, _get(cfg, "cnn_lr_decay", "linear"), _get(cfg, "cnn_learning_rate"), _get(cfg, "num_train_steps"),
                        warmup_ratio=_get(cfg, "warmup_ratio", 0.1), decay_epochs=_get(cfg, "cnn_step_decay_epochs", ()),
                        multi_step_epoch=n_epoch)
    assert len(optimizer.param_groups) == 8
    for i, pg in enumerate(optimizer.param_groups):
        if i in (0, 1):
            pg["lr"] = _get(cfg, "transformer_lr_mul", 1.0) * lr_t
        elif i in (2, 3):
            pg["lr"] = lr_t
        elif i in (4, 5):
            pg["lr"] = _get(cfg, "cnn_lr_mul", 1.0) * lr_c
        else:
            pg["lr"] = lr_c
    return lr_t, lr_c


def _mlm_masking(cfg) -> str:
    mode = _get(cfg, "mlm_masking", "host") or "host"
    if mode not in ("host", "device"):
        raise ValueError(f"mlm_masking must be 'host' or 'device', not {mode!r}")
    return mode


def _device_mlm_mask(model, ids: torch.Tensor, cfg, eval_ordinal: int):
    """cfg.mlm_masking = "device": (masked ids, labels) of the unmasked ``ids`` (mask_batch_text_tokens of src/datasets/data_utils.py:23-70
    drawn by cb_mlm_mask).  Training: a forward of its own in the runtime's count -- seed site _SITE_MLM at rt.forward_count, which then
    advances, plus the device seed word, so every eager step and every replay of a captured step masks afresh.  Evaluation: the seed of
    the ``eval_ordinal``-th batch of the pass and no seed word; no counter advances, so a validation pass repeats itself exactly."""
    from .modeling.runtime import _SITE_MLM, _seed
    rt, mc = model.rt, model.config
    if model.training:
        fwd_i = rt.forward_count
        rt.forward_count += 1
        seed, word = _seed(_SITE_MLM, 0, fwd_i), rt.seed_dev
    else:
        seed, word = _seed(_SITE_MLM, 0, int(eval_ordinal)), None
    pad = _get(mc, "pad_token_id", 0)
    return ops.mlm_mask(ids.contiguous(), float(_get(cfg, "mlm_probability", 0.15)), seed, word,
                        special_ids=tuple(_get(cfg, "mlm_special_ids", (101, 102))), pad_id=0 if pad is None else pad,
                        mask_id=int(_get(cfg, "mlm_mask_token_id", 103)), vocab_size=int(_get(mc, "vocab_size")))


def _pretrain_forward(model, batch: Dict, cfg, eval_ordinal: int = 0) -> Dict:
    """forward_step of src/pretrain/run_pretrain.py:196-202, with the masked-LM head in the mode cfg.mlm_rows names ("labelled" unless the
    config says "all"; cfg.mlm_capacity = fixed number of slots, None = every text row fits).  A batch without mlm_labels runs "all".

    cfg.mlm_masking = "device" (default "host": the caller's collator has masked the text) with cfg.use_mlm: the batch carries the UNMASKED
    text_input_ids and no mlm_labels; both are drawn here (_device_mlm_mask; ``eval_ordinal``: the batch's place in a validation pass) and
    go to the model as a host-masked batch would.  The output then also carries the masked ``text_input_ids`` that were used."""
    masking = _mlm_masking(cfg)
    mini = {k: v for k, v in batch.items() if k not in ("caption_ids", "vid_id", "question_ids")}
    mini["n_examples_list"] = list(mini["n_examples_list"])
    if not _get(cfg, "use_itm", True):
        mini["itm_labels"] = None
    drawn = masking == "device" and bool(_get(cfg, "use_mlm", True))
    if drawn:
        if mini.get("mlm_labels") is not None:
            raise ValueError("mlm_masking = 'device' draws the labels from the unmasked text_input_ids: this batch carries mlm_labels, "
                             "so its text is masked already")
        mini["text_input_ids"], mini["mlm_labels"] = _device_mlm_mask(model, mini["text_input_ids"], cfg, eval_ordinal)
    mini["mlm_rows"] = _get(cfg, "mlm_rows", "labelled") if mini.get("mlm_labels") is not None else "all"
    mini["mlm_capacity"] = _get(cfg, "mlm_capacity")
    masked_ids = mini["text_input_ids"]
    out = model(mini)
    if drawn:
        out["text_input_ids"] = masked_ids
    return out


def pretrain_loss(model, batch: Dict, cfg) -> torch.Tensor:
    """The loss of the pretraining loop (run_pretrain.py:386-395): mlm_loss.mean() if cfg.use_mlm, plus itm_loss.mean() if cfg.use_itm.
    A ``loss_fn`` for train_step / start_training."""
    out = _pretrain_forward(model, batch, cfg)
    parts = [clips.mean_loss(out[k]) for k, flag in (("mlm_loss", "use_mlm"), ("itm_loss", "use_itm"))
             if _get(cfg, flag, True) and torch.is_tensor(out[k])]
    if not parts:
        raise ValueError("pretrain_loss: neither cfg.use_mlm nor cfg.use_itm leaves a loss (or the batch carries no labels for it)")
    return parts[0] if len(parts) == 1 else parts[0] + parts[1]


def _vqa_forward(model, batch: Dict) -> Dict:
    """forward_step of src/tasks/run_vqa.py:164-169: the batch without its question ids (and without the answer types the metric reads)"""
    mini = {k: v for k, v in batch.items() if k not in ("question_ids", "answer_types")}
    mini["n_examples_list"] = list(mini["n_examples_list"])
    return model(mini)


def vqa_loss(model, batch: Dict, cfg) -> torch.Tensor:
    """The loss of the image-VQA loop (run_vqa.py:353-356): loss.mean() * num_labels of the (pairs, num_labels) BCE-with-logits loss.  A
    ``loss_fn`` for train_step / start_training / CapturedStep.  With ``answer_ids`` / ``answer_scores`` in the batch (data.
    vqa_sparse_targets) the head returns the row sums and this is their mean -- the same number; with the reference's dense ``labels`` it
    is the element-wise path times num_labels."""
    sparse = batch.get("answer_ids") is not None
    if not sparse and batch.get("labels") is None:
        raise ValueError("vqa_loss: the batch carries neither answer_ids / answer_scores nor labels")
    out = _vqa_forward(model, batch)
    if sparse:
        return clips.mean_loss(out["loss"])
    return clips.mean_loss(out["loss"].reshape(-1)) * float(out["loss"].shape[-1])


def train_step(model, optimizer, batch: Dict, cfg, global_step: int, sync=None, n_epoch: int = 0, micro_step: int = 0,
               fold_clips: bool = True, loss_fn=None) -> torch.Tensor:
    """One micro-step of start_training (:380-494): forward over the clips, pooled loss, backward; on the last micro-step of
    a gradient-accumulation group ((micro_step + 1) % cfg.gradient_accumulation_steps == 0, :426-436) also the gradient
    all-reduce (``sync`` = clipbert_amd.dist.GradSync or None), the LR schedule and clip + AdamW.  Gradients of the
    micro-steps add up un-scaled, as in the reference; the exchange happens once per group (the sum is linear).

    With ``rt.after_encoder_backward = sync.reduce_transformer`` the transformer buckets are issued from inside the LAST encoder
    backward of the group (the model counts its pending encoder nodes, so an un-folded clip loop does not fire early) and travel
    during the ResNet backward; with ``rt.after_res5_backward = sync.reduce_cnn_early`` (after ``sync.set_cnn_split``) the
    grid_encoder + res5 part of the CNN range follows from inside the last ResNet backward, while res4 / res3 still run.

    ``loss_fn``: loss = loss_fn(model, batch, cfg) replaces the clip stack and the pooled loss (pretrain_loss: the pretraining loop)."""
    acc = max(1, int(_get(cfg, "gradient_accumulation_steps", 1) or 1))
    first, last = micro_step % acc == 0, (micro_step + 1) % acc == 0
    if first:
        optimizer.zero_grad(lazy=True)                      # a backward always follows: the encoder weight gradients are overwritten
    rt = model.rt
    rt.begin_step()
    hook, hook5 = rt.after_encoder_backward, rt.after_res5_backward
    if not last:
        rt.after_encoder_backward = None                    # no exchange before the group is complete
        rt.after_res5_backward = None
    try:
        if loss_fn is not None:
            loss = loss_fn(model, batch, cfg)
        else:
            stack = forward_clips_stack(model, batch, _get(cfg, "train_n_clips", 1), _get(cfg, "num_frm"), fold=fold_clips, cfg=cfg)
            loss = training_loss(model, stack, batch["labels"], batch["n_examples_list"], _get(cfg, "score_agg_func", "mean"))
        loss.backward()
    finally:
        rt.after_encoder_backward, rt.after_res5_backward = hook, hook5
    if not last:
        return loss.detach()
    scale, g16 = 1.0, None
    if sync is not None:
        if hook is None:
            sync.reduce_transformer()
        sync.reduce_cnn()
        g16 = sync.wire_gradients()                         # bf16 wire: the optimizer reads the reduced image directly
        sync.wait(cast_back=g16 is None)
        scale = sync.grad_scale
    set_learning_rates(optimizer, cfg, global_step + 1, n_epoch)
    if sync is not None and getattr(sync, "shard", False) and sync.active:
        # owner-only update: this rank holds the reduced gradients of 1/world of every bucket (reduce-scatter), updates those pieces,
        # and the all-gather hands every rank the new compute weights
        optimizer.step(grad_scale=scale, grad16=g16, pieces=sync.owned_pieces(), norm_reduce=sync.norm_all_reduce)
        sync.gather_updated()
    else:
        optimizer.step(grad_scale=scale, grad16=g16)
    return loss.detach()


def _all_gather_scalar(x, group=None) -> list:
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return [x]
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, x, group=group)
    return parts


def _all_sum(x: float, group=None) -> float:
    """sum of a host scalar over the ranks (the reference's sum(all_gather_list(x)), :254-256)"""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return x
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, float(x), group=group)
    return float(sum(parts))


@torch.no_grad()
def validate_retrieval(model, val_loader, eval_videos, cfg, gt_txt_id2vid_id=None, group=None, on_device: bool = False) -> Dict[str, float]:
    """validate of run_video_retrieval.py:224-276: mean ITM loss / accuracy over ``val_loader`` (single-clip batches as the
    training set yields them) and the retrieval metrics of inference_retrieval over ``eval_videos``; sums over the ranks.
    ``on_device``: the metrics through inference_retrieval_matrix / eval_retrieval_matrix (every video against one caption list; ties in
    the stable order) instead of the dict rows."""
    was_training = model.training
    model.eval()
    loss, n_ex, n_correct = 0.0, 0, 0
    for batch in val_loader:
        batch = {k: v for k, v in batch.items() if k not in ("caption_ids", "vid_id")}
        targets = batch["labels"]
        out = model(dict(batch))
        if torch.is_tensor(out["loss"]):
            loss += float(out["loss"].sum().item())
        n_ex += len(targets)
        logits = out["logits"].float()
        if logits.shape[1] == 2:
            n_correct += int((logits.max(dim=-1)[1] == targets).sum().item())
        else:                                                  # rank loss: first score of each group is the positive (:244-250)
            pred = (logits > 0).long().view(out["loss"].shape[0], -1)          # sigmoid(x) > 0.5  <=>  x > 0
            n_correct += int((pred[:, 0] == targets.view(out["loss"].shape[0], -1)[:, 0]).sum().item())
    loss, n_ex, n_correct = _all_sum(loss, group), _all_sum(n_ex, group), _all_sum(n_correct, group)
    if on_device:
        matrix = inference_retrieval_matrix(model, eval_videos, cfg, group=group)
        metrics = eval_retrieval_matrix(matrix, gt_txt_id2vid_id) if gt_txt_id2vid_id is not None else None
    else:
        _rows, metrics = inference_retrieval(model, eval_videos, cfg, gt_txt_id2vid_id, group=group)
    model.train(was_training)
    log = {"valid/loss": loss / max(n_ex, 1), "valid/acc": n_correct / max(n_ex, 1)}
    for kind, m in (metrics or {}).items():
        log.update({f"valid/{kind}_{k}": round(v, 4) for k, v in m.items()})
    return log


@torch.no_grad()
def validate_pretrain(model, val_loader, cfg, group=None) -> Dict[str, float]:
    """validate of src/pretrain/run_pretrain.py:205-273: masked-LM loss / accuracy per labelled token and ITM loss / accuracy per example
    over ``val_loader``, sums over the ranks.  In the labelled-rows mode the arg-max comes from ``mlm_pred``; in "all" mode it is the
    reference's own expression on ``mlm_scores`` (:233-237).  A fixed cfg.mlm_capacity that a batch overflowed is an error here, where
    the losses are read back anyway: the dropped rows would be missing from every number.  With cfg.mlm_masking = "device" the k-th batch
    is masked from the seed of ordinal k alone: two passes over the same loader give identical numbers (what the reference's ``is_train``
    argument of mask_batch_text_tokens was kept for, data_utils.py:30, and never did)."""
    _mlm_masking(cfg)                                       # (an unknown mode is refused before the model changes its mode)
    was_training = model.training
    model.eval()
    use_mlm, use_itm = _get(cfg, "use_mlm", True), _get(cfg, "use_itm", True)
    mlm_loss, n_tok, n_tok_ok, itm_loss, n_ex, n_ex_ok = 0.0, 0, 0, 0.0, 0, 0
    for k, batch in enumerate(val_loader):
        out = _pretrain_forward(model, batch, cfg, eval_ordinal=k)      # (mlm_masking = "device": batch k of every pass draws the same masks)
        labels = out["mlm_labels"]
        if use_mlm and labels is not None:
            mlm_loss += float(out["mlm_loss"].sum().item())
            mask = labels != -100
            n_tok += int(mask.sum().item())
            if out["mlm_scores"] is None:
                if _get(cfg, "mlm_capacity") is not None and int(model.transformer.mlm_counts[1].item()) != 0:
                    raise RuntimeError(f"validate_pretrain: cfg.mlm_capacity = {_get(cfg, 'mlm_capacity')} slots dropped "
                                       f"{int(model.transformer.mlm_counts[1].item())} labelled rows")
                n_tok_ok += int((out["mlm_pred"][mask] == labels[mask]).sum().item())
            else:
                n_tok_ok += int((out["mlm_scores"][mask].max(dim=-1)[1] == labels[mask]).sum().item())
        if use_itm:
            itm_loss += float(out["itm_loss"].sum().item())
            n_ex += len(out["itm_labels"])
            n_ex_ok += int((out["itm_scores"].max(dim=-1)[1] == out["itm_labels"]).sum().item())
    mlm_loss, n_tok, n_tok_ok = _all_sum(mlm_loss, group), _all_sum(n_tok, group), _all_sum(n_tok_ok, group)
    itm_loss, n_ex, n_ex_ok = _all_sum(itm_loss, group), _all_sum(n_ex, group), _all_sum(n_ex_ok, group)
    model.train(was_training)
    log = {"valid/mlm_loss": 0, "valid/mlm_acc": 0, "valid/itm_loss": 0, "valid/itm_acc": 0}
    if n_tok != 0:
        log.update({"valid/mlm_loss": float(mlm_loss / n_tok), "valid/mlm_acc": float(n_tok_ok / n_tok)})
    if n_ex != 0:
        log.update({"valid/itm_loss": float(itm_loss / n_ex), "valid/itm_acc": float(n_ex_ok / n_ex)})
    return log


VQA_ANSWER_TYPES = ("yes/no", "number", "other")          # answer_type2idx of ClipBertVQADataset.evaluate_vqa (dataset_vqa.py:88)


def vqa_pred_scores(pred_ids: Sequence[int], ans_ids, ans_scores) -> np.ndarray:
    """float64 (n,): the VQA soft accuracy of each predicted answer id against the question's (n, K) answer tables (dataset_vqa.py:93-97:
    the annotated score of the predicted answer, 0 when it is none of them) -- on the host what cb_vqa_loss_fwd's pred_score is on the
    device"""
    ids = np.asarray(torch.as_tensor(ans_ids).cpu(), dtype=np.int64)
    sc = np.asarray(torch.as_tensor(ans_scores).cpu(), dtype=np.float64)
    pred = np.asarray(list(pred_ids), dtype=np.int64).reshape(-1, 1)
    return (sc * ((ids == pred) & (ids >= 0))).sum(axis=1)


def vqa_score_sums(scores, answer_types: Optional[Sequence[str]] = None) -> Dict[str, list]:
    """[sum of scores, count] in float64 / int for "overall" and, with ``answer_types`` (one of VQA_ANSWER_TYPES per question), for each
    type: what validate_vqa accumulates per batch and sums over the ranks"""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    sums = {"overall": [float(scores.sum()), int(scores.size)]}
    if answer_types is not None:
        types = np.asarray(list(answer_types))
        assert types.shape == scores.shape, (types.shape, scores.shape)
        unknown = set(types.tolist()) - set(VQA_ANSWER_TYPES)
        if unknown:
            raise KeyError(f"unknown answer type(s) {sorted(unknown)}: expected one of {VQA_ANSWER_TYPES}")
        for t in VQA_ANSWER_TYPES:
            sel = scores[types == t]
            sums[t] = [float(sel.sum()), int(sel.size)]
    return sums


def vqa_metrics(sums: Dict[str, list]) -> Dict[str, float]:
    """{"overall_acc", "yes/no_acc", "number_acc", "other_acc"} (those whose count is not 0) as the reference reports them:
    get_rounded_percentage of the mean score (dataset_vqa.py:99-107, run_vqa.py:220-242)"""
    return {f"{k}_acc": round(100 * (s / n), 2) for k, (s, n) in sums.items() if n}


def evaluate_vqa(pred_ids: Sequence[int], answer_types: Optional[Sequence[str]], ans_ids, ans_scores) -> Dict[str, float]:
    """ClipBertVQADataset.evaluate_vqa (dataset_vqa.py:74-112) on answer ids and the sparse tables instead of strings and the dataset's
    qid2data, in rounded percent"""
    return vqa_metrics(vqa_score_sums(vqa_pred_scores(pred_ids, ans_ids, ans_scores), answer_types))


@torch.no_grad()
def validate_vqa(model, val_loader, cfg, label2ans=None, group=None):
    """validate of src/tasks/run_vqa.py:172-257 -> (rows, log).  rows: dict(question_id, answer) per question, answer =
    label2ans[predicted id] (the id itself without ``label2ans``).  log["valid/loss"] = the summed loss / the number of questions.  Batches
    with ``answer_ids`` / ``answer_scores`` take loss, arg-max and the score of the arg-max from the fused head and also yield
    valid/overall_acc and -- where they carry an ``answer_types`` list -- valid/yes/no_acc, valid/number_acc, valid/other_acc, each
    round(100 * x, 2) (get_rounded_percentage); dense ``labels`` give the loss only; batches without answers (test sets) give the rows
    from logits.max(dim=-1)[1] and no scores.  Score sums and counts are kept on the host in float64 and summed over the ranks: exact
    sums where the reference re-weights per-rank means (:223-242), the same value up to rounding."""
    was_training = model.training
    model.eval()
    rows, loss, n_ex = [], 0.0, 0
    sums = {k: [0.0, 0] for k in ("overall",) + VQA_ANSWER_TYPES}
    for batch in val_loader:
        out = _vqa_forward(model, batch)
        n = out["logits"].shape[0]
        qids = batch.get("question_ids", list(range(n_ex, n_ex + n)))
        if torch.is_tensor(out["loss"]):
            loss += float(out["loss"].sum().item())
        n_ex += n
        if "pred" in out:
            pred = out["pred"].tolist()
            part = vqa_score_sums(out["pred_score"].double().cpu().numpy(), batch.get("answer_types"))
            for k, (s, c) in part.items():
                sums[k][0] += s
                sums[k][1] += c
        else:
            pred = out["logits"].max(dim=-1)[1].tolist()
        rows.extend(dict(question_id=q, answer=label2ans[p] if label2ans is not None else p) for q, p in zip(qids, pred))
    loss, n_ex = _all_sum(loss, group), _all_sum(n_ex, group)
    sums = {k: [_all_sum(s, group), _all_sum(c, group)] for k, (s, c) in sums.items()}
    model.train(was_training)
    log = {"valid/loss": float(loss / max(n_ex, 1))}
    log.update({f"valid/{k}": v for k, v in vqa_metrics(sums).items()})
    return rows, log


def start_training(model, optimizer, train_loader, cfg, sync=None, validate_fn=None, model_saver=None, restorer=None,
                   total_n_examples: Optional[int] = None, fold_clips: bool = True, log_fn=None, overlap: bool = True, loss_fn=None,
                   capture=False) -> int:
    """The loop of start_training (run_video_retrieval.py:379-516 / run_video_qa.py:457-560) around train_step: infinite
    iteration over ``train_loader`` until cfg.num_train_steps optimizer steps, gradient accumulation, LR schedules with the
    multi-step epoch counter, validation + ``model_step_N.pt`` every cfg.valid_steps (and once at the end), restorer.step()
    after every optimizer step.  ``train_loader`` yields collated batches (clipbert_amd.data.PrefetchLoader delivers them with
    uint8 frames already in HBM).  With several ranks and ``overlap`` the gradient exchange is armed to leave from inside the
    backward (GradSync.attach).  Returns the final global step.

    Ranks: pass ``model_saver`` / ``restorer`` on EVERY rank (clipbert_amd.checkpoint: both write on rank 0 only, the restorer
    restores on all ranks -- the reference's order, run_video_retrieval.py:329-346).  All ranks must run the same number of
    optimizer steps: the resumed global step is agreed on across the ranks (max), and when the ranks did not all restore the
    same step, the most advanced rank's parameters, AdamW moments and optimizer step count are broadcast before the first step.

    ``loss_fn``: handed to every train_step (see there).

    ``capture``: False (default) = every step is the eager train_step.  True = the steps go through clipbert_amd.captured.CapturedStep:
    a batch signature seen twice is captured as a hipGraph and replayed from then on, everything a graph must not freeze falls back to
    train_step with a warning (see that module).  "dry" = its bookkeeping without graphs (tests), or pass a CapturedStep built by the
    caller (``max_graphs``, ``pad_text_to``, ``raw_frames``) on the SAME model, optimizer, loss_fn, fold_clips and sync (checked); it is
    used as it is.  cfg.capture_raw_frames = 1 (default 0) builds the stepper with ``raw_frames=True``: data.RawFrames batches replay as
    well, read where the loader put them (their bytes are never staged; the stepper keeps the batch's buffer alive until the next one)."""
    from .data import InfiniteIterator
    stepper = None
    if capture:
        from .captured import CapturedStep
        if isinstance(capture, CapturedStep):
            stepper = capture
            differ = [n for n, v in (("model", model), ("optimizer", optimizer), ("loss_fn", loss_fn), ("sync", sync)) if getattr(stepper, n) is not v]
            if bool(stepper.fold_clips) != bool(fold_clips):
                differ.append("fold_clips")
            if differ:                                      # (e.g. an object without the loop's multi-rank sync would capture a step without the exchange)
                raise ValueError(f"start_training(capture=CapturedStep): the object was built with another {' / '.join(differ)} than the loop was called with")
        else:
            stepper = CapturedStep(model, optimizer, cfg, loss_fn=loss_fn, fold_clips=fold_clips, sync=sync, mode="dry" if capture == "dry" else "graph",
                                   raw_frames=bool(_get(cfg, "capture_raw_frames", 0)))
    if sync is not None and sync.world > 1 and overlap and model.rt is not None and model.rt.after_encoder_backward is None:
        sync.attach(model)
    acc = max(1, int(_get(cfg, "gradient_accumulation_steps", 1) or 1))
    global_step = restorer.global_step if restorer is not None else 0
    if sync is not None and sync.world > 1 and not sync.dry:
        steps = _all_gather_scalar(global_step)
        if len(set(steps)) > 1:
            # the ranks resumed from different states (e.g. restore.pt readable on one rank only): ALL of them continue from the most
            # advanced one -- its global step, parameters, AdamW moments and optimizer step count (the reference broadcasts both
            # model and optimizer state from rank 0 after its restore, run_video_retrieval.py:304-305,329-346)
            global_step = int(max(steps))
            src = steps.index(global_step)
            if restorer is not None:
                restorer.global_step = global_step
            sync.broadcast_state(optimizer, src)
    num_train_steps, valid_steps = int(_get(cfg, "num_train_steps")), int(_get(cfg, "valid_steps", 0) or 0)
    n_gpu = sync.world if sync is not None else 1
    total_bsz = n_gpu * int(_get(cfg, "train_batch_size", 1)) * acc * int(_get(cfg, "max_n_example_per_group", 1) or 1)
    model.train()

    sharded = sync is not None and getattr(sync, "shard", False) and sync.active

    def run_validation(step):
        if validate_fn is not None:
            log = validate_fn(model, step)
            if log_fn is not None and log is not None:
                log_fn(step, log)
        if model_saver is not None:
            if sharded:
                sync.gather_state(optimizer)                # (every rank: the fp32 masters and moments return from their owners)
            model_saver.save(step=step, model=model)

    if global_step >= num_train_steps:
        return global_step
    for micro, batch in enumerate(InfiniteIterator(train_loader)):
        n_epoch = int(1.0 * total_bsz * (global_step + 1) / total_n_examples) if total_n_examples else 0
        if stepper is not None:
            loss = stepper.step(batch, global_step, n_epoch=n_epoch, micro_step=micro)
        else:
            loss = train_step(model, optimizer, batch, cfg, global_step, sync=sync, n_epoch=n_epoch, micro_step=micro, fold_clips=fold_clips,
                              loss_fn=loss_fn)
        if (micro + 1) % acc != 0:
            continue
        global_step += 1
        if log_fn is not None:
            log_fn(global_step, {"train/loss": float(loss.item()) if global_step % 50 == 0 else None})
        if restorer is not None:
            if sharded and (restorer.global_step + 1) % restorer.save_steps == 0:
                sync.gather_state(optimizer)                # restore.pt is written by this step()
            restorer.step()
        if valid_steps and global_step % valid_steps == 0:
            run_validation(global_step)
        if global_step >= num_train_steps:
            break
    if not valid_steps or global_step % valid_steps != 0:
        run_validation(global_step)
    return global_step


# ---- retrieval inference (:628-734) ------------------------------------------------------------------------------------
@torch.no_grad()
def inference_retrieval_video(model, visual_inputs: torch.Tensor, text_input_ids: torch.Tensor, text_input_mask: torch.Tensor,
                              cfg, cache_cnn: bool = True, max_pairs_per_pass: int = 256, capture=None) -> List[float]:
    """Scores of ONE video (1, inference_n_clips*num_frm, 3, H, W) against all its candidate captions (:640-690).

    cache_cnn=True (row N1): the grid features of all clips are computed once, in one CNN batch, and every text
    mini-batch runs only the cross-modal encoder -- on several clips at once (pairs = clips x captions, at most
    ``max_pairs_per_pass`` per encoder pass: measured on MI355X, an encoder batch whose activations outgrow the 256 MB
    Infinity Cache (1024 pairs = 42 k token rows: 258 MB per FFN activation) runs its GEMMs 3-5x slower per row than a
    batch of a few thousand rows).  cache_cnn=False is the reference's order of evaluation (full forward per clip per
    mini-batch).  Both give the same scores.

    ``capture``: None / False (default) = eager encoder passes.  A clipbert_amd.captured.CapturedForward = the encoder passes replay from
    its hipGraphs (one full and one remainder signature per video set; the CNN pass stays eager); True = the one kept on the model
    (created on first use), so that the graphs outlive the call.  cache_cnn=True only."""
    scores: List[float] = []
    for _i0, pooled in _retrieval_video_pooled(model, visual_inputs, text_input_ids, text_input_mask, cfg, cache_cnn, max_pairs_per_pass, capture):
        scores.extend(clips.retrieval_scores(pooled))
    return scores


def _retrieval_video_pooled(model, visual_inputs, text_input_ids, text_input_mask, cfg, cache_cnn, max_pairs_per_pass, capture):
    """The passes of inference_retrieval_video: yields (first caption, pooled logits (nb, C)) per text mini-batch, on the device; what
    becomes of them -- rounded host floats, or a slice of a score-matrix row -- is the caller's."""
    if capture:
        from .captured import CapturedForward
        if not cache_cnn:
            raise ValueError("inference_retrieval_video(capture=...) replays the encoder passes over cached grid features: cache_cnn=True only")
        if not isinstance(capture, CapturedForward):
            if getattr(model, "_captured_forward", None) is None:
                model._captured_forward = CapturedForward(model, mode="dry" if capture == "dry" else "graph")
            capture = model._captured_forward
    n_clips, num_frm = _get(cfg, "inference_n_clips", 1), _get(cfg, "num_frm")
    pool, eval_bsz = _get(cfg, "score_agg_func", "mean"), _get(cfg, "inference_batch_size", 64)
    vis = visual_inputs.view(n_clips, num_frm, *visual_inputs.shape[2:])
    n_txt = text_input_ids.shape[0]
    grid = model.grid_features(vis) if cache_cnn else None          # (n_clips, T, H', W', hidden)
    for i0 in range(0, n_txt, eval_bsz):
        ids, mask = text_input_ids[i0:i0 + eval_bsz], text_input_mask[i0:i0 + eval_bsz]
        nb = ids.shape[0]
        if cache_cnn:
            cpp = max(1, min(n_clips, max_pairs_per_pass // max(nb, 1)))          # clips per encoder pass
            per_clip = []
            for c0 in range(0, n_clips, cpp):
                nc = min(cpp, n_clips - c0)
                if capture:
                    lg = capture.logits(grid[c0:c0 + nc], ids.repeat(nc, 1), mask.repeat(nc, 1), [nb] * nc)
                else:
                    lg = model.forward_from_grid(dict(visual_inputs=grid[c0:c0 + nc], text_input_ids=ids.repeat(nc, 1),
                                                      text_input_mask=mask.repeat(nc, 1), labels=None,
                                                      n_examples_list=[nb] * nc))["logits"]
                per_clip.extend(lg.view(nc, nb, -1).unbind(0))
        else:
            per_clip = []
            for c in range(n_clips):
                out = model(dict(visual_inputs=vis[c:c + 1], text_input_ids=ids, text_input_mask=mask, labels=None,
                                 n_examples_list=[nb]))
                per_clip.append(out["logits"])
        pooled = clips.aggregate_clip_logits(per_clip, pool)
        if pool == "lse":
            pooled = clips.lse_inference_logits(pooled)
        yield i0, pooled


def shard_for_rank(n_items: int, rank: int, world: int) -> range:
    """Items (videos) of this rank: a strided partition, what DistributedSampler(shuffle=False) hands out without padding
    (no duplicated videos: the reference's eval_retrieval drops duplicates anyway, :574-577)."""
    return range(rank, n_items, world)


def gather_retrieval_rows(rows: List[Dict], group=None) -> List[Dict]:
    """All ranks' dict(vid_id, txt_id, score) rows on every rank, in rank order -- the exchange the reference does through
    per-rank JSON files on shared storage (:696-724); here ONE all-gather of a compact (ids, float32 scores) payload.
    Works on RCCL ("nccl") and gloo groups; a single process returns its rows unchanged."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return rows
    payload = ([r["vid_id"] for r in rows], [r["txt_id"] for r in rows], np.asarray([r["score"] for r in rows], dtype=np.float64))
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, payload, group=group)
    out: List[Dict] = []
    for vids, txts, sc in parts:
        out.extend(dict(vid_id=v, txt_id=t, score=float(x)) for v, t, x in zip(vids, txts, sc))
    return out


@torch.no_grad()
def inference_retrieval(model, videos, cfg, gt_txt_id2vid_id: Optional[Dict] = None, group=None, cache_cnn: bool = True, capture=False):
    """inference_retrieval of the reference (:628-734) for the videos of THIS rank: ``videos`` yields dict(vid_id,
    visual_inputs (1, n_clips*num_frm, 3, H, W), text_input_ids, text_input_mask, caption_ids) -- one video against all its
    candidate captions.  Returns (rows of all ranks, metrics or None); videos are independent units, the only exchange is
    the final gather of the score rows.  ``capture``: handed to every inference_retrieval_video (see there)."""
    was_training = model.training
    model.eval()
    rows: List[Dict] = []
    for b in videos:
        scores = inference_retrieval_video(model, b["visual_inputs"], b["text_input_ids"], b["text_input_mask"], cfg, cache_cnn=cache_cnn,
                                           capture=capture or None)
        rows.extend(dict(vid_id=b["vid_id"], txt_id=c, score=s) for c, s in zip(b["caption_ids"], scores))
    rows = gather_retrieval_rows(rows, group)
    metrics = eval_retrieval(rows, gt_txt_id2vid_id) if gt_txt_id2vid_id is not None else None
    model.train(was_training)
    return rows, metrics


# ---- retrieval evaluation on the device (:563-734 without per-batch host traffic) ----------------------------------------------------
class RetrievalMatrix:
    """The scores of an evaluation as ONE video-major matrix: ``scores`` fp32 (len(vid_ids), len(txt_ids)) on the device, not rounded
    (cb_retrieval_rank rounds to the exact integer keys); row i is video ``vid_ids[i]``, column j caption ``txt_ids[j]``."""

    def __init__(self, vid_ids: List, txt_ids: List, scores: torch.Tensor):
        assert scores.dim() == 2 and tuple(scores.shape) == (len(vid_ids), len(txt_ids)) and scores.dtype == torch.float32
        self.vid_ids, self.txt_ids, self.scores = list(vid_ids), list(txt_ids), scores


def merge_retrieval_parts(parts):
    """The per-rank (vid_ids, txt_ids, fp32 numpy block (videos, captions)) triples as one: the rows concatenated in rank order, a repeated
    vid_id dropped (the first occurrence stays, as eval_retrieval does, :578-586).  Every part must name the same captions in the same
    order.  A pure function of its argument."""
    parts = list(parts)
    txt_ids = list(parts[0][1])
    vid_ids, blocks, seen = [], [], set()
    for rank, (vids, txts, block) in enumerate(parts):
        if list(txts) != txt_ids:
            raise ValueError(f"merge_retrieval_parts: rank {rank} scored other captions than rank 0 (the matrix path needs every video "
                             "compared with the same caption list: inference_retrieval is the general path)")
        block = np.asarray(block, dtype=np.float32).reshape(len(vids), len(txt_ids))
        keep = []
        for i, v in enumerate(vids):
            if v not in seen:
                seen.add(v)
                keep.append(i)
                vid_ids.append(v)
        blocks.append(block if len(keep) == len(vids) else block[keep])
    return vid_ids, txt_ids, np.concatenate(blocks, axis=0)


def gather_retrieval_matrix(local: RetrievalMatrix, group=None) -> RetrievalMatrix:
    """All ranks' rows on every rank, in rank order: ONE all_gather_object of (vid_ids, txt_ids, fp32 numpy block) per rank -- 4 bytes a
    score where gather_retrieval_rows pickles a dict entry.  A single process returns its matrix unchanged."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, (local.vid_ids, local.txt_ids, local.scores.cpu().numpy()), group=group)
    vid_ids, txt_ids, block = merge_retrieval_parts(parts)
    return RetrievalMatrix(vid_ids, txt_ids, torch.from_numpy(block).to(local.scores.device))


@torch.no_grad()
def inference_retrieval_matrix(model, videos, cfg, group=None, cache_cnn: bool = True, capture=False, max_pairs_per_pass: int = 256) -> RetrievalMatrix:
    """inference_retrieval without the dict rows: the same encoder passes, pooling and cb_retrieval_scores launches as
    inference_retrieval_video (bit-identical fp32 scores), every mini-batch's scores written straight into its slice of the video's row of a
    device matrix -- nothing is copied to the host inside the loop.  ``videos`` as for inference_retrieval; every video must carry the
    same ``caption_ids`` sequence (MSRVTT 1k-A: each video against all captions), else ValueError -- inference_retrieval is the general
    path.  A repeated vid_id is skipped, the first occurrence stays (:578-586).  Returns the matrix of all ranks (gather_retrieval_matrix)."""
    was_training = model.training
    model.eval()
    vid_ids, seen, txt_ids, scores = [], set(), None, None
    for b in videos:
        caption_ids = list(b["caption_ids"])
        if txt_ids is None:
            txt_ids = caption_ids
            capacity = max(len(videos), 1) if hasattr(videos, "__len__") else 16
            scores = torch.empty(capacity, len(txt_ids), dtype=torch.float32, device=b["text_input_ids"].device)
        elif caption_ids != txt_ids:
            raise ValueError(f"inference_retrieval_matrix: video {b['vid_id']!r} carries other caption_ids than the first video; the score "
                             "matrix needs one caption list for all videos -- use inference_retrieval, the general path")
        if b["vid_id"] in seen:
            continue
        if len(vid_ids) == scores.shape[0]:                 # (an iterable without a length: the matrix grows on the device)
            scores = torch.cat([scores, torch.empty_like(scores)])
        row = scores[len(vid_ids)]
        for i0, pooled in _retrieval_video_pooled(model, b["visual_inputs"], b["text_input_ids"], b["text_input_mask"], cfg, cache_cnn,
                                                  max_pairs_per_pass, capture or None):
            ops.retrieval_scores(pooled.float().contiguous(), out=row[i0:i0 + pooled.shape[0]])
        seen.add(b["vid_id"])
        vid_ids.append(b["vid_id"])
    model.train(was_training)
    if txt_ids is None:
        raise ValueError("inference_retrieval_matrix: no videos")
    return gather_retrieval_matrix(RetrievalMatrix(vid_ids, txt_ids, scores[:len(vid_ids)]), group)


def retrieval_metrics_from_ranks(ranks) -> Dict[str, float]:
    """get_retrieval_metric_from_bool_matrix (:519-543) from the 1-based ranks of the ground truths: the reference's expressions, float64."""
    ranks = np.asarray(ranks, dtype=np.int64)
    num_row = len(ranks)
    return dict(r1=float(100 * (ranks <= 1).sum() / num_row), r5=float(100 * (ranks <= 5).sum() / num_row),
                r10=float(100 * (ranks <= 10).sum() / num_row), medianR=float(np.median(ranks)), meanR=float(np.mean(ranks)))


def eval_retrieval_matrix(matrix: RetrievalMatrix, gt_txt_id2vid_id: Dict) -> Dict[str, Dict[str, float]]:
    """eval_retrieval (:563-625) on a RetrievalMatrix: the ground-truth index arrays built on the host as eval_retrieval builds them (the
    video -> text ground truth is the inverse dict, so the LAST caption of a video wins, :618), one copy of them to the device, two
    cb_retrieval_rank launches and one copy of both rank vectors back.  Ties: the stable order (ops.retrieval_rank)."""
    vid_idx = {v: i for i, v in enumerate(matrix.vid_ids)}
    txt_idx = {t: i for i, t in enumerate(matrix.txt_ids)}
    gt_v2t = {v: t for t, v in gt_txt_id2vid_id.items()}
    gt_cols = [vid_idx[gt_txt_id2vid_id[t]] for t in matrix.txt_ids]          # text -> video: per caption, its video's row
    gt_rows = [txt_idx[gt_v2t[v]] for v in matrix.vid_ids]                    # video -> text: per video, its caption's column
    gt = torch.tensor(gt_cols + gt_rows, dtype=torch.int32).to(matrix.scores.device)
    n_txt = len(gt_cols)
    r_t2v = ops.retrieval_rank(matrix.scores, gt[:n_txt], ops.RANK_COL_QUERIES)
    r_v2t = ops.retrieval_rank(matrix.scores, gt[n_txt:], ops.RANK_ROW_QUERIES)
    ranks = torch.cat([r_t2v, r_v2t]).cpu().numpy()
    return dict(text2video=retrieval_metrics_from_ranks(ranks[:n_txt]), video2text=retrieval_metrics_from_ranks(ranks[n_txt:]))


def retrieval_rows(matrix: RetrievalMatrix) -> List[Dict]:
    """The reference's list of dict(vid_id, txt_id, score) (:683-688) from a RetrievalMatrix, for saving results: video-major, score =
    key / 1e4 -- the double round(p, 4) gives.  Built only when asked for: one launch for the keys, one copy to the host."""
    if not matrix.vid_ids or not matrix.txt_ids:
        return []
    no_gt = torch.full((len(matrix.vid_ids),), -1, dtype=torch.int32).to(matrix.scores.device)      # (rank 0 everywhere: only the keys are wanted)
    _rank, keys = ops.retrieval_rank(matrix.scores, no_gt, ops.RANK_ROW_QUERIES, want_keys=True)
    keys = keys.cpu().tolist()
    return [dict(vid_id=v, txt_id=t, score=k / 1e4) for v, row in zip(matrix.vid_ids, keys) for t, k in zip(matrix.txt_ids, row)]


# ---- MSRVTT multiple-choice test (run_msrvtt_mc.py:136-243) ----------------------------------------------------------------
_AGG_MODES = {"mean": ops.AGG_MEAN, "max": ops.AGG_MAX, "lse": ops.AGG_LSE}


def _agg_mode(pool_method: str) -> int:
    if pool_method not in _AGG_MODES:                       # (the runner raises ValueError too, :186-188)
        raise ValueError(f"cfg.score_agg_func must be one of {sorted(_AGG_MODES)}, not {pool_method!r}")
    return _AGG_MODES[pool_method]


@torch.no_grad()
def mc_clip_logits(model, batch: Dict, cfg, n_options: int = 5, cache_cnn: bool = True, max_pairs_per_pass: int = 256,
                   capture=None) -> torch.Tensor:
    """The clip loop of the multiple-choice test (:165-178) -> the fp32 (inference_n_clips, B*n_options, C) stack of per-clip logits, on
    the device.  ``batch`` has the keys of MSRVTTMCCollator (data.collate_mc): visual_inputs (B, n_clips*num_frm, 3, H, W),
    text_input_ids / text_input_mask (B*n_options, L) -- video v's options are rows v*n_options .. -- and n_examples_list == [1]*B.

    cache_cnn=False is the reference's order of evaluation: one full model(batch) per clip with n_examples_list multiplied by n_options
    (forward_step, :136-142).  cache_cnn=True (default) runs ONE CNN batch over all B*n_clips clips and then only the cross-modal encoder,
    over runs of (clip, video) blocks of n_options pairs each, at most ``max_pairs_per_pass`` pairs per pass (the reasoning and the
    default of inference_retrieval_video); the passes walk the blocks clip-major, so their logits concatenate into the stack as they
    come.  ``capture``: as in inference_retrieval_video -- None / False, True (the CapturedForward kept on the model), "dry", or a
    CapturedForward; the encoder passes then replay from its graphs (one full and one remainder signature per batch shape).
    cache_cnn=True only."""
    if capture:
        from .captured import CapturedForward
        if not cache_cnn:
            raise ValueError("mc_clip_logits(capture=...) replays the encoder passes over cached grid features: cache_cnn=True only")
        if not isinstance(capture, CapturedForward):
            if getattr(model, "_captured_forward", None) is None:
                model._captured_forward = CapturedForward(model, mode="dry" if capture == "dry" else "graph")
            capture = model._captured_forward
    n_clips, num_frm, n_options = int(_get(cfg, "inference_n_clips", 1)), int(_get(cfg, "num_frm")), int(n_options)
    vis, ids, mask = batch["visual_inputs"], batch["text_input_ids"], batch["text_input_mask"]
    counts = list(batch["n_examples_list"])
    bsz = len(counts)
    if any(e != 1 for e in counts) or vis.shape[0] != bsz or ids.shape[0] != bsz * n_options:
        raise ValueError(f"mc_clip_logits: expected one question of {n_options} options per video, got n_examples_list {counts}, "
                         f"{vis.shape[0]} videos and {ids.shape[0]} text rows")
    if not cache_cnn:
        vis = vis.view(bsz, n_clips, num_frm, *vis.shape[2:])
        per_clip = []
        for c in range(n_clips):
            mini = dict(visual_inputs=vis[:, c].contiguous() if n_clips > 1 else vis[:, 0], text_input_ids=ids, text_input_mask=mask,
                        labels=None, n_examples_list=[e * n_options for e in counts])
            per_clip.append(model(mini)["logits"])
        return torch.stack(per_clip).float()
    grid = model.grid_features(vis.view(bsz * n_clips, num_frm, *vis.shape[2:]))      # row v*n_clips + c: the plain view, no copy
    if n_clips > 1 and bsz > 1:                                                         # clip-major blocks: row c*bsz + v
        grid = grid.reshape(bsz, n_clips, *grid.shape[1:]).transpose(0, 1).reshape(bsz * n_clips, *grid.shape[1:])
    ids3, mask3 = ids.view(bsz, n_options, -1), mask.view(bsz, n_options, -1)
    n_blocks = n_clips * bsz
    per_pass = max(1, int(max_pairs_per_pass) // n_options)                              # (clip, video) blocks per encoder pass
    parts = []
    for j0 in range(0, n_blocks, per_pass):
        j1 = min(j0 + per_pass, n_blocks)
        seg_ids, seg_mask, j = [], [], j0
        while j < j1:                                                                   # the videos of blocks j0..j1-1: runs of v = j % bsz
            v = j % bsz
            take = min(bsz - v, j1 - j)
            seg_ids.append(ids3[v:v + take])
            seg_mask.append(mask3[v:v + take])
            j += take
        p_ids = (seg_ids[0] if len(seg_ids) == 1 else torch.cat(seg_ids)).reshape((j1 - j0) * n_options, -1)
        p_mask = (seg_mask[0] if len(seg_mask) == 1 else torch.cat(seg_mask)).reshape((j1 - j0) * n_options, -1)
        if capture:
            lg = capture.logits(grid[j0:j1], p_ids, p_mask, [n_options] * (j1 - j0))
        else:
            lg = model.forward_from_grid(dict(visual_inputs=grid[j0:j1], text_input_ids=p_ids, text_input_mask=p_mask, labels=None,
                                              n_examples_list=[n_options] * (j1 - j0)))["logits"]
        parts.append(lg)
    lg = parts[0] if len(parts) == 1 else torch.cat(parts)
    return lg.float().reshape(n_clips, bsz * n_options, -1)


@torch.no_grad()
def mc_predict_batch(model, batch: Dict, cfg, n_options: int = 5, cache_cnn: bool = True, max_pairs_per_pass: int = 256, capture=None):
    """(pred int32 (B,), scores fp32 (B*n_options,)) of one batch, both on the device: mc_clip_logits, then the pooling over the clips
    (cfg.score_agg_func), the probability and the arg-max over each question's options in one launch (ops.mc_predict; :178-195).  No
    host synchronisation."""
    mode = _agg_mode(_get(cfg, "score_agg_func", "mean"))
    stack = mc_clip_logits(model, batch, cfg, n_options=n_options, cache_cnn=cache_cnn, max_pairs_per_pass=max_pairs_per_pass, capture=capture)
    scores, pred = ops.mc_predict(stack, n_options, mode)
    return pred, scores


def gather_mc_predictions(pred_id2ans: Dict, group=None) -> Dict:
    """The {question id: predicted option} dicts of all ranks merged on every rank, in rank order -- the exchange the reference does
    through per-rank JSON files on shared storage and merge_dicts (:202-234); here ONE all_gather_object.  A single process returns its
    dict unchanged."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return pred_id2ans
    parts = [None] * dist.get_world_size(group)
    dist.all_gather_object(parts, (list(pred_id2ans.keys()), list(pred_id2ans.values())), group=group)
    merged: Dict = {}
    for keys, values in parts:
        merged.update(zip(keys, values))
    return merged


def mc_accuracy(pred_id2ans: Dict, id2answer: Dict, force_same: bool = True) -> Dict[str, str]:
    """ClipBertMSRVTTMCEvalDataset.evaluate_qa_accuracy (src/datasets/dataset_video_retrieval.py:307-325) on the ground-truth dict
    instead of the dataset: with ``force_same`` the predictions must name exactly the ground truth's ids (asserted), without it every
    predicted id is looked up.  Returns dict(mc_accuracy="<percent, 2 decimals>")."""
    if force_same:
        assert set(id2answer) == set(pred_id2ans), "the predictions and the ground truth name different question ids"
    hits = np.asarray([int(id2answer[k]) == int(a) for k, a in pred_id2ans.items()], dtype=bool)
    acc = np.mean(hits)                                     # (no predictions: nan, as the reference's mean of an empty array)
    return dict(mc_accuracy=f"{100 * acc:.2f}")


@torch.no_grad()
def inference_retrieval_mc(model, val_loader, cfg, n_options: int = 5, id2answer: Optional[Dict] = None, group=None, cache_cnn: bool = True,
                           capture=False):
    """inference_retrieval_mc of the reference (:145-243) over the batches of THIS rank -> (pred_id2ans of all ranks, metrics or None).
    ``val_loader`` yields the batches of data.collate_mc (``question_ids`` names each video's question; an ``answers`` entry is not
    read).  The predictions stay on the device until the loader is exhausted: one concatenation and one .tolist() bring them to the
    host.  ``id2answer`` ({question id: index of the right option}, of ALL ranks' questions) gives metrics = mc_accuracy(...);
    ``capture``: handed to every mc_clip_logits (see there).  The model is put in eval mode for the loop and returned to its mode."""
    was_training = model.training
    model.eval()
    qids: List = []
    preds: List[torch.Tensor] = []
    for batch in val_loader:
        q = list(batch["question_ids"])
        assert len(q) == len(batch["n_examples_list"]), (len(q), len(batch["n_examples_list"]))
        pred, _scores = mc_predict_batch(model, batch, cfg, n_options=n_options, cache_cnn=cache_cnn, capture=capture or None)
        qids.extend(q)
        preds.append(pred)
    answers = (preds[0] if len(preds) == 1 else torch.cat(preds)).tolist() if preds else []
    pred_id2ans = {q: int(a) for q, a in zip(qids, answers)}
    pred_id2ans = gather_mc_predictions(pred_id2ans, group)
    metrics = mc_accuracy(pred_id2ans, id2answer, force_same=True) if id2answer is not None else None
    model.train(was_training)
    return pred_id2ans, metrics


# ---- video QA inference (run_video_qa.py:216-300) ------------------------------------------------------------------------
@torch.no_grad()
def qa_predict(model, batch: Dict, cfg, fold_clips: bool = False) -> List[int]:
    """Predicted answer ids of one batch: clip loop over inference_n_clips, pooling, then argmax (classification tasks
    action / transition / frameqa / msrvtt_qa) or round-and-clamp to 1..10 (the regression task "count").

    fold_clips=True (row N1 for QA): all clips of all videos go through the CNN and the encoder as ONE batch -- (clip, video)
    pairs become the "videos" of a single forward -- instead of inference_n_clips separate forwards; same predictions."""
    n_clips, num_frm = _get(cfg, "inference_n_clips", 1), _get(cfg, "num_frm")
    if fold_clips and n_clips > 1:
        vis = batch["visual_inputs"]
        bsz = vis.shape[0]
        vis = vis.view(bsz, n_clips, num_frm, *vis.shape[2:]).transpose(0, 1).reshape(n_clips * bsz, num_frm, *vis.shape[2:])
        counts = _pair_counts(cfg, batch["n_examples_list"])
        out = model(dict(visual_inputs=vis.contiguous(), text_input_ids=batch["text_input_ids"].repeat(n_clips, 1),
                         text_input_mask=batch["text_input_mask"].repeat(n_clips, 1), labels=None, n_examples_list=counts * n_clips))
        lg = out["logits"]
        logits = list(lg.view(n_clips, lg.shape[0] // n_clips, *lg.shape[1:]).unbind(0))
    else:
        logits = forward_clips(model, dict(batch, labels=None), n_clips, num_frm, fold=False, cfg=cfg)
    pool = _get(cfg, "score_agg_func", "mean")
    pooled = clips.aggregate_clip_logits(logits, pool)
    if pool == "lse":
        pooled = clips.lse_inference_logits(pooled)
    if _get(cfg, "task", "action") in ("action", "transition", "frameqa", "msrvtt_qa"):
        return pooled.max(dim=-1)[1].tolist()
    return (pooled + 0.5).long().clamp(min=1, max=10).reshape(-1).tolist()


@torch.no_grad()
def validate_qa(model, val_loader, cfg, group=None, fold_clips: bool = True):
    """validate of run_video_qa.py:216-362 without the dataset-specific score tables: per batch the pooled prediction of
    qa_predict over cfg.inference_n_clips clips -> rows dict(question_id, answer); with labels in the batch also the overall
    accuracy (classification tasks) / mean absolute error rounded as the reference reports it (count), summed over ranks."""
    was_training = model.training
    model.eval()
    rows, n_ex, n_hit, abs_err = [], 0, 0, 0.0
    for batch in val_loader:
        qids = batch.get("question_ids", list(range(n_ex, n_ex + len(batch["n_examples_list"]))))
        b = {k: v for k, v in batch.items() if k != "question_ids"}
        pred = qa_predict(model, b, cfg, fold_clips=fold_clips)
        rows.extend(dict(question_id=q, answer=a) for q, a in zip(qids, pred))
        if batch.get("labels") is not None:
            gt = batch["labels"].view(-1).tolist()
            n_ex += len(gt)
            n_hit += sum(int(a == int(g)) for a, g in zip(pred, gt))
            abs_err += sum(abs(a - g) for a, g in zip(pred, gt))
    n_ex, n_hit, abs_err = _all_sum(n_ex, group), _all_sum(n_hit, group), _all_sum(abs_err, group)
    model.train(was_training)
    log = {}
    if n_ex:
        log = {"valid/overall_acc": round(100.0 * n_hit / n_ex, 2)} if _get(cfg, "task", "action") != "count" else {"valid/mae": round(abs_err / n_ex, 2)}
    return rows, log


# ---- video QA validation on the device (run_video_qa.py:216-362, dataset_video_qa.py:131-183) ------------------------------------------
QA_MC_TASKS = ("action", "transition")                     # one text row per (question, option) pair
QA_CLASSIFY_TASKS = QA_MC_TASKS + ("frameqa", "msrvtt_qa")  # arg-max answers; everything else ("count") is the clamped regression
QA_ANSWER_TYPES = dict(frameqa=("object", "number", "color", "location"),          # answer_type2idx of evaluate_tgif_qa (:147-150)
                       msrvtt_qa=("what", "who", "how", "where", "when"))


@torch.no_grad()
def qa_clip_logits(model, batch: Dict, cfg, cache_cnn: bool = True, max_pairs_per_pass: int = 256, capture=None) -> torch.Tensor:
    """The clip loop of the QA validation (:245-261) -> the fp32 (inference_n_clips, B, C) stack of per-clip logits, on the device.  ``batch``
    has the keys of VideoQACollator (data.collate_qa) with ONE question per video, as the validation loaders are built (:98); anything
    else raises ValueError.  action / transition: cfg.num_labels text rows per video, C = cfg.num_labels (the head's view(-1, num_labels));
    frameqa / msrvtt_qa / count: one text row per video, C = the head's width.  This is mc_clip_logits -- the same CNN batch, encoder passes
    of at most ``max_pairs_per_pass`` pairs over clip-major (clip, video) blocks and ``capture`` choices; cache_cnn=False is the
    reference's order, one full forward per clip with forward_step's multiplied counts (:206-210) -- with the task's rows per video.  The
    batch's labels are not passed into the model."""
    n_options = int(_get(cfg, "num_labels")) if _get(cfg, "task", "action") in QA_MC_TASKS else 1
    stack = mc_clip_logits(model, batch, cfg, n_options=n_options, cache_cnn=cache_cnn, max_pairs_per_pass=max_pairs_per_pass, capture=capture)
    return stack.reshape(stack.shape[0], len(batch["n_examples_list"]), -1)


@torch.no_grad()
def qa_predict_batch(model, batch: Dict, cfg, cache_cnn: bool = True, max_pairs_per_pass: int = 256, capture=None):
    """(pred int32 (B,), loss fp32 (B,) | None) of one batch, both on the device: qa_clip_logits, then the pooling over the clips
    (cfg.score_agg_func), the answer (:273-279) and -- with batch["labels"] -- each question's loss, the mean over the clips of its
    per-clip cross entropy / squared error (what :250-259 sums), in one launch (ops.qa_predict).  No host synchronisation."""
    mode = _agg_mode(_get(cfg, "score_agg_func", "mean"))
    count = _get(cfg, "task", "action") not in QA_CLASSIFY_TASKS
    stack = qa_clip_logits(model, batch, cfg, cache_cnn=cache_cnn, max_pairs_per_pass=max_pairs_per_pass, capture=capture)
    labels = batch.get("labels")
    if labels is not None:
        labels = torch.as_tensor(labels).reshape(-1).to(device=stack.device, dtype=torch.float32 if count else torch.int32).contiguous()
    pred, loss, _pooled = ops.qa_predict(stack, mode, kind=ops.QA_COUNT if count else ops.QA_CLASSIFY, labels=labels)
    return pred, loss


def video_qa_counters(pred, gt, answer_types: Optional[Sequence[str]], task: str, loss_sum: float = 0.0) -> Dict:
    """The additive counters of one rank: n, hits, abs_err (the sum of |pred - gt|: the count task's error), loss_sum and, for frameqa /
    msrvtt_qa with ``answer_types`` (one of QA_ANSWER_TYPES[task] per question), type_n / type_hits per type.  ``pred`` / ``gt``: integer
    arrays (answer ids, options or counts; a ground truth outside the vocabulary is any id no prediction takes, e.g. -1)."""
    p, g = np.asarray(pred, dtype=np.int64).reshape(-1), np.asarray(gt, dtype=np.int64).reshape(-1)
    assert p.shape == g.shape, (p.shape, g.shape)
    hit = p == g
    c = dict(n=int(p.size), hits=int(hit.sum()), abs_err=int(np.abs(p - g).sum()), loss_sum=float(loss_sum))
    if task in QA_ANSWER_TYPES and answer_types is not None:
        types = np.asarray(list(answer_types))
        assert types.shape == p.shape, (types.shape, p.shape)
        unknown = set(types.tolist()) - set(QA_ANSWER_TYPES[task])
        if unknown:
            raise KeyError(f"unknown answer type(s) {sorted(unknown)}: expected one of {QA_ANSWER_TYPES[task]}")
        c["type_n"] = {t: int((types == t).sum()) for t in QA_ANSWER_TYPES[task]}
        c["type_hits"] = {t: int(hit[types == t].sum()) for t in QA_ANSWER_TYPES[task]}
    return c


def merge_video_qa_counters(parts: Sequence[Dict]) -> Dict:
    """the counters of several ranks (or batches) added up, in the order given"""
    out = dict(n=0, hits=0, abs_err=0, loss_sum=0.0)
    for c in parts:
        for k in ("n", "hits", "abs_err", "loss_sum"):
            out[k] += c[k]
        for k in ("type_n", "type_hits"):
            if k in c:
                tgt = out.setdefault(k, {})
                for t, v in c[k].items():
                    tgt[t] = tgt.get(t, 0) + v
    return out


def video_qa_metrics(counters: Dict, task: str, per_rank: bool = False) -> Dict:
    """The score dict from (merged) counters.  per_rank=True: what evaluate_tgif_qa returns for one rank (dataset_video_qa.py:167-183) --
    overall_acc and the per-type *_acc as fractions (0 for an empty type), ratios = {type_ratio: [share, count]}.  per_rank=False: the
    gathered scores of validate (:304-348) -- the accuracies as get_rounded_percentage (round(100 x, 2); count: round(x, 2)), ratios =
    {type_ratio: [rounded percentage of all questions, count]} -- from exact integer sums where the reference re-weights per-rank means:
    the same value up to rounding."""
    n = counters["n"]
    classify = task in QA_CLASSIFY_TASKS

    def shown(x):
        return x if per_rank else (round(x * 100, 2) if classify else round(x, 2))

    scores = dict(overall_acc=shown(counters["hits"] / n if n else float("nan")))      # (np.mean of nothing is nan in the reference too)
    if "type_n" in counters:
        ratios = {}
        for t, cnt in counters["type_n"].items():
            scores[f"{t}_acc"] = shown(counters["type_hits"][t] / cnt) if cnt else 0
            share = 1. * cnt / n
            ratios[f"{t}_ratio"] = [share if per_rank else round(share * 100, 2), cnt]
        scores["ratios"] = ratios
    return scores


def video_qa_scores(pred, gt, answer_types: Optional[Sequence[str]], task: str) -> Dict:
    """ClipBertVideoQADataset.evaluate_tgif_qa (dataset_video_qa.py:131-183) for one rank, on integer arrays and a list of answer-type names
    instead of the dataset's qid2data: overall_acc, and for frameqa / msrvtt_qa the per-type *_acc and ratios."""
    return video_qa_metrics(video_qa_counters(pred, gt, answer_types, task), task, per_rank=True)


@torch.no_grad()
def validate_video_qa(model, val_loader, cfg, qid2data: Optional[Dict] = None, label2ans: Optional[Dict] = None, eval_score: bool = True,
                      group=None, cache_cnn: bool = True, capture=False, val_log: Optional[Dict] = None):
    """validate of run_video_qa.py:216-362 over the batches of THIS rank -> (qa_results, gathered_scores).  ``val_loader`` yields the
    batches of data.collate_qa.  Per batch one qa_predict_batch; predictions, losses and labels stay on the device until the loader is
    exhausted, then one concatenation and one transfer bring them to the host.  qa_results: dict(question_id, answer: the int the
    reference stores, and data=qid2data[qid] when ``qid2data`` is given) per question of this rank.  gathered_scores (eval_score=True):
    video_qa_metrics of the counters of all ranks, merged through one all_gather_object; the ground truth is qid2data[qid]["answer"] /
    ["answer_type"] when ``qid2data`` is given (frameqa / msrvtt_qa: answer strings, mapped through ``label2ans`` {id: answer} as the
    reference maps the predictions), else batch["labels"] and batch.get("answer_types").  eval_score=False (test sets without answers):
    gathered_scores == 0.  ``val_log`` (a dict, optional) receives what the reference logs: valid/loss -- the summed loss over the number
    of questions, 0 without labels -- and one valid/<k> per non-ratio score.  ``capture``: handed to every qa_clip_logits.  The model is
    put in eval mode for the loop and returned to its mode."""
    task = _get(cfg, "task", "action")
    was_training = model.training
    model.eval()
    try:
        qids: List = []
        types: List = []
        packed: List[torch.Tensor] = []
        have_loss = have_labels = True
        for batch in val_loader:
            q = list(batch["question_ids"])
            assert len(q) == len(batch["n_examples_list"]), (len(q), len(batch["n_examples_list"]))
            pred, loss = qa_predict_batch(model, {k: v for k, v in batch.items() if k not in ("question_ids", "answer_types")}, cfg,
                                          cache_cnn=cache_cnn, capture=capture or None)
            labels = batch.get("labels")
            have_loss, have_labels = have_loss and loss is not None, have_labels and labels is not None
            zero = torch.zeros_like(pred)
            lab = zero if labels is None else torch.as_tensor(labels).reshape(-1).to(device=pred.device, dtype=torch.int32)
            packed.append(torch.stack([pred, zero if loss is None else loss.view(torch.int32), lab]))       # (the loss travels as its bits)
            qids.extend(q)
            if batch.get("answer_types") is not None:
                types.extend(batch["answer_types"])
        host = (packed[0] if len(packed) == 1 else torch.cat(packed, dim=1)).cpu() if packed else torch.zeros(3, 0, dtype=torch.int32)
    finally:
        model.train(was_training)
    answers = host[0].tolist()
    loss_sum = float(host[1].view(torch.float32).double().sum()) if have_loss else 0.0
    qa_results = [dict(question_id=q, answer=a, **({} if qid2data is None else dict(data=qid2data[q]))) for q, a in zip(qids, answers)]
    n_ex = len(qids)
    if not eval_score:
        total = merge_video_qa_counters(_all_gather_scalar(dict(n=n_ex, hits=0, abs_err=0, loss_sum=loss_sum), group))
        gathered_scores = 0
    else:
        if qid2data is not None:
            gt, types = [qid2data[q]["answer"] for q in qids], [qid2data[q].get("answer_type") for q in qids]
            if task in QA_ANSWER_TYPES:                     # answer strings -> ids; an answer outside the vocabulary matches no prediction
                if label2ans is None:
                    raise ValueError(f"validate_video_qa: the ground truth of task {task!r} is an answer string: label2ans is needed")
                ans2label = {v: int(k) for k, v in label2ans.items()}
                gt = [ans2label.get(g, -1) for g in gt]
        elif have_labels:
            gt = host[2].tolist()
        else:
            raise ValueError("validate_video_qa(eval_score=True) needs the answers: qid2data, or labels in every batch")
        use_types = types if task in QA_ANSWER_TYPES and len(types) == n_ex and n_ex else None
        total = merge_video_qa_counters(_all_gather_scalar(video_qa_counters(answers, gt, use_types, task, loss_sum), group))
        gathered_scores = video_qa_metrics(total, task)
    if val_log is not None:
        val_log["valid/loss"] = float(total["loss_sum"] / total["n"]) if total["n"] else float("nan")
        if eval_score:
            val_log.update({f"valid/{k}": v for k, v in gathered_scores.items() if "ratio" not in k})
    return qa_results, gathered_scores


# ---- metrics (:519-625) ------------------------------------------------------------------------------------------------
def retrieval_metrics_from_scores(score_matrix, gt_cols: Sequence[int]) -> Dict[str, float]:
    """score_matrix (#queries, #candidates), gt_cols[i] = index of query i's ground-truth candidate -> recall@{1,5,10} in %,
    median and mean rank (1-indexed); ties keep the order of a stable descending sort like torch.sort."""
    sm = torch.as_tensor(score_matrix, dtype=torch.float32)
    order = torch.sort(sm, dim=1, descending=True)[1]
    gt = torch.as_tensor(list(gt_cols)).view(-1, 1)
    ranks = (order == gt).float().argmax(dim=1).numpy() + 1
    n = float(len(ranks))
    return dict(r1=100.0 * float((ranks <= 1).sum()) / n, r5=100.0 * float((ranks <= 5).sum()) / n,
                r10=100.0 * float((ranks <= 10).sum()) / n, medianR=float(np.median(ranks)), meanR=float(np.mean(ranks)))


def eval_retrieval(vid_txt_score_dicts: List[Dict], gt_txt_id2vid_id: Dict) -> Dict[str, Dict[str, float]]:
    """Same contract as the reference's eval_retrieval (:563-625): rows of dict(vid_id, txt_id, score) -> text2video and
    video2text metric dicts (first occurrence of a (txt, vid) pair wins; every caption must see the same videos)."""
    by_txt = defaultdict(dict)
    for d in vid_txt_score_dicts:
        by_txt[d["txt_id"]].setdefault(d["vid_id"], d["score"])
    txt_ids = list(by_txt)
    vid_ids = list(by_txt[txt_ids[0]])
    for t in txt_ids:
        assert len(by_txt[t]) == len(vid_ids), "each captions should be compared with the same #videos."
    vid_idx = {v: i for i, v in enumerate(vid_ids)}
    sm = torch.zeros(len(txt_ids), len(vid_ids))
    for r, t in enumerate(txt_ids):
        for v, s in by_txt[t].items():
            sm[r, vid_idx[v]] = s
    t2v = retrieval_metrics_from_scores(sm, [vid_idx[gt_txt_id2vid_id[t]] for t in txt_ids])
    txt_idx = {t: i for i, t in enumerate(txt_ids)}
    gt_v2t = {v: t for t, v in gt_txt_id2vid_id.items()}
    v2t = retrieval_metrics_from_scores(sm.t(), [txt_idx[gt_v2t[v]] for v in vid_ids])
    return dict(text2video=t2v, video2text=v2t)


def qa_accuracy(pred_ids: Sequence[int], gt_ids: Sequence[int]) -> float:
    """answer id = argmax of the pooled logits (run_video_qa.py:273-275); accuracy in %."""
    p, g = np.asarray(list(pred_ids)), np.asarray(list(gt_ids))
    return 100.0 * float((p == g).mean()) if len(g) else math.nan
