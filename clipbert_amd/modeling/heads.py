"""Task heads: small autograd nodes (one consumer each, so autograd never has to add tensors), loss nodes, the five task models."""
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..ops import ACT_GELU, ACT_NONE, ACT_RELU, KROW, KROW_GATHER, ROWK_GATHER
from .cnn import conv_gather
from .encoder import ClipBertBaseModel, _drop_p, _linear_wgrad
from .modules import BatchNorm1d, Linear, _cfg_get, _make_mlp, _PreTrainingHeads, as_config
from .runtime import _SITE_REG, Runtime, _seed


def _row_gather(rt, operand, rows, k, device):
    """gather block of ``rows`` = (n_seg, seg_len, seg_stride_rows) of a (*, k) matrix: n_seg one-row images of seg_len pixels"""
    nseg, seglen, segstride = rows
    return conv_gather(rt, operand, nseg, 1, seglen, k, 1, 1, 0, device, sN=segstride * k, sH=0)


def _slot_gather(operand, sel, k):
    """the same block for the ``sel.cap`` rows of a (*, k) matrix that cb_mlm_select picked on the device: its table instead of a host-built one"""
    kw = dict(R=1, S=1, Cin=k, H=1, W=sel.lt, sH=0, sW=k)
    kw.update(dict(a_mode=ROWK_GATHER, a_tab=sel.tab, lda=0) if operand == "a" else dict(b_mode=KROW_GATHER, b_tab=sel.tab, ldb=0))
    return kw


def _gather(rt, operand, rows, k, device):
    return _slot_gather(operand, rows, k) if isinstance(rows, ops.MlmSelection) else _row_gather(rt, operand, rows, k, device)


class _LinearFn(torch.autograd.Function):
    """y = act(x W^T + b).  ``rows`` = (n_seg, seg_len, seg_stride_rows) selects x rows (b*stride + t); an ops.MlmSelection selects the
    rows its device-built table names (padding slots read zeros; their gradient rows land in a dump row that is cut off)."""
    @staticmethod
    def forward(ctx, anchor, x, rt, weight, bias, act, out_f32, rows):
        n, k = weight.shape
        dev = x.device
        x2 = x.reshape(-1, k)
        slots = isinstance(rows, ops.MlmSelection)
        m = x2.shape[0] if rows is None else rows.cap if slots else rows[0] * rows[1]
        gather = {} if rows is None else _gather(rt, "a", rows, k, dev)
        out_dt = torch.float32 if out_f32 else rt.dtype
        ld = n if n < 4 else (n + 3) // 4 * 4              # (1- / 2-column head outputs stay contiguous: the losses read them in place)
        store = torch.empty(m, ld, dtype=out_dt, device=dev)
        y = store[:, :n]
        save = ctx.needs_input_grad[0]
        pre = torch.empty(m, ld, dtype=rt.dtype, device=dev)[:, :n] if (save and act == ACT_GELU) else None
        ops.gemm(x2, rt.bank.compute(weight), m, n, k, out=y, **gather, shift=bias, act=act, out2=pre)
        ctx.rt, ctx.weight, ctx.bias, ctx.act, ctx.rows = rt, weight, bias, act, rows
        ctx.x2, ctx.y, ctx.pre, ctx.m, ctx.x_shape = (x2 if save else None), (y if save else None), pre, m, x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        rt, weight, bias, act = ctx.rt, ctx.weight, ctx.bias, ctx.act
        bank, dt = rt.bank, rt.dtype
        n, k = weight.shape
        m = ctx.m
        g = dy
        if g.dtype != dt or g.stride(1) != 1:
            g = ops.cast(g.contiguous(), torch.empty(m, n, dtype=dt, device=dy.device))
        if act == ACT_GELU:
            g = ops.act_bwd(ACT_GELU, g.contiguous(), ctx.pre.contiguous())
        elif act != ACT_NONE:
            g = ops.act_bwd(act, g.contiguous(), ctx.y.contiguous().to(dt))
        x2, rows = ctx.x2, ctx.rows
        gb = _linear_wgrad(g, x2, m, n, k, bank.grad_image(weight), bank.grad_image(bias) if bias is not None else None,
                           gather=None if rows is None else _gather(rt, "b", rows, k, dy.device), defer_bias=True)
        if rows is None:
            dx, rowmap = torch.empty(x2.shape, dtype=dt, device=dy.device), None
        elif isinstance(rows, ops.MlmSelection):        # (one dump row behind the real ones takes the padding slots' zeros)
            dx, rowmap = ops.zeros((x2.shape[0] + 1, k), dt, dy.device), rows.rowmap
        else:                                           # (rows outside the segments get no gradient)
            dx, rowmap = ops.zeros(x2.shape, dt, dy.device), rt.strided_rowmap(rows[0], 1, rows[2], 1, rows[1], 1, dy.device)
        ops.gemm(g, bank.compute(weight), m, k, n, out=dx, lda=g.stride(0), b_mode=KROW, c_rowmap=rowmap)
        if gb is not None:
            ops.colsum(g, gb, m, n)
        return None, dx[:x2.shape[0]].view(ctx.x_shape), None, None, None, None, None, None


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, x, rt, ln):
        save = ctx.needs_input_grad[0]
        xc = x.contiguous()
        y, mean, rstd = ops.layernorm_fwd(xc, ln.weight, ln.bias, ln.eps, save_stats=save)
        ctx.rt, ctx.ln, ctx.saved = rt, ln, (xc, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, mean, rstd = ctx.saved
        bank = ctx.rt.bank
        dx, _ = ops.layernorm_bwd(dy.contiguous(), xc, ctx.ln.weight, mean, rstd, bank.grad_image(ctx.ln.weight),
                                  bank.grad_image(ctx.ln.bias))
        return None, dx, None, None


class _CrossEntropyFn(torch.autograd.Function):
    """CrossEntropyLoss(reduction='none', ignore_index=-100) on fp32 logits (rows, C)."""
    @staticmethod
    def forward(ctx, logits, labels):
        loss, _ = ops.cross_entropy(logits, labels)
        ctx.save_for_backward(logits, labels)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, labels = ctx.saved_tensors
        _, dlogits = ops.cross_entropy(logits, labels, want_loss=False, dloss=dloss.contiguous(), want_grad=True)
        return dlogits, None


class _MlmDecoderLossFn(torch.autograd.Function):
    """Tied decoder (transformers.py:504-515) + masked-LM loss and arg-max (modeling.py:287-298, run_pretrain.py:229-237) on the ``sel.cap``
    compact rows: fp32 logits (cap, V) -> per-row loss (B * Lt,), zeros at unlabelled rows; the arg-max lands in sel.pred_rows.  ONE node
    for the two stages: autograd converts a gradient to the dtype of the tensor it belongs to, so fp32 logits handed from a decoder node
    to a loss node would bring back the fp32 gradient matrix and the cast that cb_mlm_loss_bwd exists to avoid."""
    @staticmethod
    def forward(ctx, anchor, h, rt, weight, bias, sel):
        n, k = weight.shape
        m = sel.cap
        logits = torch.empty(m, (n + 3) // 4 * 4, dtype=torch.float32, device=h.device)[:, :n]
        ops.gemm(h, rt.bank.compute(weight), m, n, k, out=logits, shift=bias, act=ACT_NONE)
        lse = ops.mlm_loss_fwd(logits, sel)
        ctx.rt, ctx.weight, ctx.bias, ctx.sel, ctx.saved = rt, weight, bias, sel, (h, logits, lse)
        return sel.loss_rows

    @staticmethod
    def backward(ctx, dloss):
        rt, weight, bias, sel = ctx.rt, ctx.weight, ctx.bias, ctx.sel
        h, logits, lse = ctx.saved
        bank = rt.bank
        n, k = weight.shape
        m = sel.cap
        g = ops.mlm_loss_bwd(logits, lse, sel, dloss.contiguous(), rt.dtype)
        gb = _linear_wgrad(g, h, m, n, k, bank.grad_image(weight), bank.grad_image(bias), defer_bias=True)
        dh = torch.empty(h.shape, dtype=rt.dtype, device=h.device)
        ops.gemm(g, bank.compute(weight), m, k, n, out=dh, lda=g.stride(0), b_mode=KROW)
        if gb is not None:
            ops.colsum(g, gb, m, n)
        return None, dh, None, None, None, None


class _VqaHeadLossFn(torch.autograd.Function):
    """Last classifier Linear (modeling.py:338-343) + the BCE-with-logits loss of the VQA head on SPARSE answers (modeling.py:310-316,
    372-374; the targets of dataset_vqa.py:57-72 as (pairs, K) id / score tables): fp32 logits (pairs, C) -> per-pair loss (pairs,) = the
    row sums of the reference's (pairs, C) loss, with the arg-max and its VQA score (run_vqa.py:188, dataset_vqa.py:93-97) from the same
    pass.  ONE node for the two stages, for the reason _MlmDecoderLossFn gives: cb_vqa_loss_bwd writes the gradient once, in the compute
    dtype, as the A operand of the two backward GEMMs."""
    @staticmethod
    def forward(ctx, anchor, h, rt, weight, bias, ans_ids, ans_scores):
        n, k = weight.shape
        h2 = h.reshape(-1, k)
        m = h2.shape[0]
        logits = torch.empty(m, (n + 3) // 4 * 4, dtype=torch.float32, device=h.device)[:, :n]
        ops.gemm(h2, rt.bank.compute(weight), m, n, k, out=logits, shift=bias, act=ACT_NONE)
        loss, pred, score = ops.vqa_loss_fwd(logits, ans_ids, ans_scores)
        ctx.rt, ctx.weight, ctx.bias, ctx.saved, ctx.h_shape = rt, weight, bias, (h2, logits, ans_ids, ans_scores), h.shape
        ctx.mark_non_differentiable(logits, pred, score)
        ctx.set_materialize_grads(False)                 # (no zero matrix for the logits' absent gradient)
        return loss, logits, pred, score

    @staticmethod
    def backward(ctx, dloss, _dlogits, _dpred, _dscore):
        if dloss is None:
            return (None,) * 7
        rt, weight, bias = ctx.rt, ctx.weight, ctx.bias
        h2, logits, ans_ids, ans_scores = ctx.saved
        bank = rt.bank
        n, k = weight.shape
        m = h2.shape[0]
        g = ops.vqa_loss_bwd(logits, ans_ids, ans_scores, dloss.contiguous(), rt.dtype)
        gb = _linear_wgrad(g, h2, m, n, k, bank.grad_image(weight), bank.grad_image(bias) if bias is not None else None, defer_bias=True)
        dh = torch.empty(h2.shape, dtype=rt.dtype, device=h2.device)
        ops.gemm(g, bank.compute(weight), m, k, n, out=dh, lda=g.stride(0), b_mode=KROW)
        if gb is not None:
            ops.colsum(g, gb, m, n)
        return None, dh.view(ctx.h_shape), None, None, None, None, None


class _HeadLossFn(torch.autograd.Function):
    """Element-wise head losses of the reference through cb_head_loss (reduction "none"): MSE (num_labels == 1), BCE with logits (VQA-style
    soft targets), sigmoid margin ranking of the retrieval head -- src/modeling/modeling.py:359-381, 431-446, 567-575."""
    @staticmethod
    def forward(ctx, logits, targets, kind, group, margin):
        loss, _ = ops.head_loss(kind, logits, targets, group=group, margin=margin)
        ctx.save_for_backward(logits, targets)
        ctx.args = (kind, group, margin)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, targets = ctx.saved_tensors
        kind, group, margin = ctx.args
        _, dx = ops.head_loss(kind, logits, targets, want_loss=False, dloss=dloss.contiguous().float(), want_grad=True, group=group, margin=margin)
        return dx, None, None, None, None


def head_loss_none(kind: int, logits: torch.Tensor, targets: Optional[torch.Tensor] = None, group: int = 1, margin: float = 0.0) -> torch.Tensor:
    lg = (logits if logits.dtype == torch.float32 else logits.float()).contiguous()
    tg = None if targets is None else targets.to(torch.float32).contiguous()
    return _HeadLossFn.apply(lg, tg, kind, group, margin)


def cross_entropy_none(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    lg = logits if logits.dtype == torch.float32 else logits.float()
    return _CrossEntropyFn.apply(lg, labels.contiguous())


class _ClipBertHead(nn.Module):
    """Common part of the task models: owns ``bert`` and the runtime; pooled output -> _head (the ``classifier`` MLP) -> calc_loss."""
    def __init__(self, config):
        super().__init__()
        config = as_config(config)
        self.config = config
        self.bert = ClipBertBaseModel(config)
        self.rt: Optional[Runtime] = None

    def forward(self, text_input_ids, visual_inputs, text_input_mask, labels=None, src_row=None, text_repeat=1, **loss_args):
        _, pooled = self.bert(text_input_ids, visual_inputs, text_input_mask, src_row, pooled_dropout=True, text_repeat=text_repeat)
        logits, loss = self.calc_loss(self._head(pooled), labels, **loss_args)
        return dict(logits=logits, loss=loss)

    def _head(self, pooled):
        rt, (fc1, _, fc2) = self.rt, self.classifier
        h = _LinearFn.apply(rt.anchor, pooled, rt, fc1.weight, fc1.bias, ACT_RELU, False, None)
        return _LinearFn.apply(rt.anchor, h, rt, fc2.weight, fc2.bias, ACT_NONE, True, None)

    def calc_loss(self, logits, labels):
        """the MSE / BCE / CE ladder of the sequence-classification and multiple-choice heads (modeling.py:359-381, 431-446)"""
        if labels is None:
            return logits, 0
        if self.config.num_labels == 1:
            return logits, head_loss_none(ops.LOSS_MSE, logits.reshape(-1), labels.reshape(-1))
        if self.config.loss_type == "bce":
            return logits, head_loss_none(ops.LOSS_BCE, logits, labels)
        if self.config.loss_type == "ce":
            return logits, cross_entropy_none(logits.view(-1, self.config.num_labels), labels.view(-1))
        raise ValueError("Invalid option for config.loss_type")


class ClipBertForVideoTextRetrieval(_ClipBertHead):
    """src/modeling/modeling.py:523-580."""
    def __init__(self, config):
        super().__init__(config)
        self.classifier = _make_mlp(self.config.hidden_size, self.config.num_labels)
        self.margin = _cfg_get(self.config, "margin", 0.0)

    def forward(self, text_input_ids, visual_inputs, text_input_mask, labels=None, sample_size=-1, src_row=None, text_repeat=1):
        return super().forward(text_input_ids, visual_inputs, text_input_mask, labels, src_row, text_repeat, sample_size=sample_size)

    def calc_loss(self, logits, labels, sample_size=-1):
        if labels is None:
            return logits, 0
        if self.config.loss_type == "ce":
            loss = cross_entropy_none(logits.view(-1, self.config.num_labels), labels.view(-1))
        elif self.config.loss_type == "rank":
            # sigmoid margin ranking, modeling.py:567-575: rows of (1 positive + negatives) scores per video
            assert sample_size > 0
            group = logits.numel() // sample_size
            if group < 2:                      # no negatives: the reference's scores[:, 1:] is (B, 0) and so is its loss (modeling.py:572-575)
                loss = logits.new_zeros((sample_size, 0), dtype=torch.float32)
            else:
                loss = head_loss_none(ops.LOSS_RANK, logits.reshape(sample_size, -1), group=group, margin=self.margin)
        else:
            raise ValueError("Invalid option for config.loss_type")
        return logits, loss


class ClipBertForMultipleChoice(_ClipBertHead):
    """src/modeling/modeling.py:387-451."""
    def __init__(self, config):
        super().__init__(config)
        self.classifier = _make_mlp(self.config.hidden_size, 1)

    def calc_loss(self, logits, labels):
        if self.config.loss_type != "ce":
            return super().calc_loss(logits, labels)
        logits = logits.reshape(-1, self.config.num_labels)            # (also what comes back without labels)
        return logits, super().calc_loss(logits.contiguous(), labels)[1]


class ClipBertForSequenceClassification(_ClipBertHead):
    """src/modeling/modeling.py:327-384."""
    def __init__(self, config):
        super().__init__(config)
        self.classifier = _make_mlp(self.config.hidden_size, self.config.num_labels)

    def forward(self, text_input_ids, visual_inputs, text_input_mask, labels=None, src_row=None, text_repeat=1, answer_ids=None,
                answer_scores=None):
        """``answer_ids`` int32 / ``answer_scores`` fp32 (pairs, K) (data.vqa_sparse_targets: padding id -1): the VQA targets kept sparse.
        The last classifier Linear and the loss then run as one node and the call returns dict(logits, loss (pairs,): the ROW SUMS of the
        dense path's (pairs, num_labels) loss, pred (pairs,) int64: the arg-max, pred_score (pairs,) fp32: its VQA soft accuracy).
        Without them: the dense ``labels`` path, unchanged."""
        if answer_ids is None and answer_scores is None:
            return super().forward(text_input_ids, visual_inputs, text_input_mask, labels, src_row, text_repeat)
        if answer_ids is None or answer_scores is None:
            raise ValueError("answer_ids and answer_scores come together")
        if labels is not None:
            raise ValueError("sparse answers (answer_ids / answer_scores) and dense labels exclude each other")
        if self.config.loss_type != "bce" or self.config.num_labels <= 1:
            raise ValueError(f"sparse answers need loss_type 'bce' and num_labels > 1, not {self.config.loss_type!r} / {self.config.num_labels}")
        _, pooled = self.bert(text_input_ids, visual_inputs, text_input_mask, src_row, pooled_dropout=True, text_repeat=text_repeat)
        rt, (fc1, _, fc2) = self.rt, self.classifier
        h = _LinearFn.apply(rt.anchor, pooled, rt, fc1.weight, fc1.bias, ACT_RELU, False, None)
        loss, logits, pred, score = _VqaHeadLossFn.apply(rt.anchor, h, rt, fc2.weight, fc2.bias, answer_ids.to(torch.int32).contiguous(),
                                                         answer_scores.to(torch.float32).contiguous())
        return dict(logits=logits, loss=loss, pred=pred, pred_score=score)


class _EluBnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, x, rt, bn, training):
        xc = x.contiguous()
        y, sm, si = ops.elu_bn1d_fwd(xc, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, bn.momentum, bn.eps, save=True)
        if training:
            bn.num_batches_tracked += 1
        ctx.rt, ctx.bn, ctx.training, ctx.saved = rt, bn, training, (xc, sm, si)
        return y

    @staticmethod
    def backward(ctx, dy):
        xc, sm, si = ctx.saved
        bank, bn = ctx.rt.bank, ctx.bn
        dx = ops.elu_bn1d_bwd(dy.contiguous(), xc, bn.weight, sm, si, bank.grad_image(bn.weight), bank.grad_image(bn.bias), ctx.training)
        return None, dx, None, None, None


class ClipBertForRegression(_ClipBertHead):
    """src/modeling/modeling.py:454-507: pooled -> dropout -> Linear -> ELU -> BatchNorm1d -> dropout -> Linear(1); MSE loss.
    (No runner of the reference instantiates it -- the TGIF "count" task goes through ClipBertForSequenceClassification with
    num_labels = 1 -- but it is part of the module API.)"""
    def __init__(self, config):
        super().__init__(config)
        d = self.config.hidden_size
        self.regressor = nn.ModuleList([Linear(d, d), nn.Identity(), BatchNorm1d(d), nn.Identity(), Linear(d, 1)])

    def _head(self, pooled):
        rt, reg = self.rt, self.regressor
        h = _LinearFn.apply(rt.anchor, pooled, rt, reg[0].weight, reg[0].bias, ACT_NONE, False, None)
        h = _EluBnFn.apply(rt.anchor, h, rt, reg[2], self.training)
        p = _drop_p(self, self.training)
        if p > 0:
            h = _DropoutFn.apply(h, rt, p, rt.forward_count)
        return _LinearFn.apply(rt.anchor, h, rt, reg[4].weight, reg[4].bias, ACT_NONE, True, None)

    def calc_loss(self, logits, labels):
        if labels is None:
            return logits, 0
        if self.config.loss_type == "mse":
            return logits, head_loss_none(ops.LOSS_MSE, logits.reshape(-1), labels.reshape(-1))
        raise ValueError(f"Invalid option {self.config.loss_type} for config.loss_type")


class _DropoutFn(torch.autograd.Function):
    """nn.Dropout on a small head activation (the regression head's second dropout): stateless hash mask, same in backward"""
    @staticmethod
    def forward(ctx, x, rt, p, fwd_i):
        ctx.rt, ctx.p, ctx.seed = rt, p, _seed(_SITE_REG, 0, fwd_i)
        return ops.dropout(x.contiguous(), p, ctx.seed, rt.seed_dev)

    @staticmethod
    def backward(ctx, dy):
        return ops.dropout(dy.contiguous(), ctx.p, ctx.seed, ctx.rt.seed_dev), None, None, None


class ClipBertForPreTraining(_ClipBertHead):
    """src/modeling/modeling.py:241-307 with BertPreTrainingHeads (transformers.py:479-547)."""
    def __init__(self, config):
        super().__init__(config)
        self.cls = _PreTrainingHeads(self.config, self.bert.embeddings.word_embeddings.weight)
        self.mlm_counts: Optional[torch.Tensor] = None    # device [count, dropped] of the labelled-rows mode (forward)

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    def labelled_mlm_head(self, seq, lt, mlm_labels, mlm_capacity=None):
        """The masked-LM head on the labelled text rows of the (B, L, d) encoder output only: cb_mlm_select -> transform dense + GELU on the
        gathered rows -> LayerNorm -> tied decoder -> loss + arg-max, every matrix ``cap`` rows tall.  -> (loss (B * Lt,), pred (B, Lt))"""
        rt, pred = self.rt, self.cls.predictions
        b, L, d = seq.shape
        cap = (max(1, b * lt if mlm_capacity is None else int(mlm_capacity)) + 63) // 64 * 64
        if self.mlm_counts is None or self.mlm_counts.device != seq.device:
            self.mlm_counts = ops.zeros(2, torch.int64, seq.device)
        sel = ops.mlm_select(mlm_labels.reshape(-1).contiguous(), lt, L, d, self.config.vocab_size, cap, counts=self.mlm_counts)
        h = _LinearFn.apply(rt.anchor, seq, rt, pred.transform.dense.weight, pred.transform.dense.bias, ACT_GELU, False, sel)
        h = _LayerNormFn.apply(rt.anchor, h, rt, pred.transform.LayerNorm)
        loss = _MlmDecoderLossFn.apply(rt.anchor, h, rt, pred.decoder.weight, pred.bias, sel)
        return loss, sel.pred_rows.view(b, lt)

    def forward(self, text_input_ids, visual_inputs, text_input_mask, mlm_labels=None, itm_labels=None, src_row=None, mlm_rows="all",
                mlm_capacity=None):
        """``mlm_rows`` = "labelled": the masked-LM head runs on the labelled text rows only (cb_mlm_select compacts them on the device
        into ``mlm_capacity`` slots, rounded up to 64; None = every text row fits): ``mlm_scores`` is None, ``mlm_loss`` is the same
        (B * Lt,) vector, and ``mlm_pred`` (B, Lt) holds the arg-max at labelled positions, -100 elsewhere.  self.mlm_counts (device
        int64: [labelled rows of the last call, rows dropped so far for want of slots]) tells a caller whether a fixed capacity held."""
        if mlm_rows not in ("all", "labelled"):
            raise ValueError(f"mlm_rows must be 'all' or 'labelled', not {mlm_rows!r}")
        if mlm_rows == "labelled" and mlm_labels is None:
            raise ValueError("mlm_rows='labelled' needs mlm_labels")
        rt = self.rt
        seq, pooled = self.bert(text_input_ids, visual_inputs, text_input_mask, src_row)
        b, L, d = seq.shape
        lt = text_input_mask.shape[1]
        pred = self.cls.predictions
        rel = self.cls.seq_relationship
        v = self.config.vocab_size
        if mlm_rows == "labelled":
            mlm_loss, mlm_pred = self.labelled_mlm_head(seq, lt, mlm_labels, mlm_capacity)
            itm = _LinearFn.apply(rt.anchor, pooled, rt, rel.weight, rel.bias, ACT_NONE, True, None)
            itm_loss = cross_entropy_none(itm.view(-1, 2), itm_labels.view(-1)) if itm_labels is not None else 0
            return dict(mlm_scores=None, mlm_loss=mlm_loss, mlm_labels=mlm_labels, itm_scores=itm, itm_loss=itm_loss,
                        itm_labels=itm_labels, mlm_pred=mlm_pred)
        # heads on the TEXT rows only (modeling.py:283-285): gathered inside the GEMM loader
        h = _LinearFn.apply(rt.anchor, seq, rt, pred.transform.dense.weight, pred.transform.dense.bias, ACT_GELU, False,
                            (b, lt, L))
        h = _LayerNormFn.apply(rt.anchor, h, rt, pred.transform.LayerNorm)
        scores = _LinearFn.apply(rt.anchor, h, rt, pred.decoder.weight, pred.bias, ACT_NONE, True, None)
        itm = _LinearFn.apply(rt.anchor, pooled, rt, rel.weight, rel.bias, ACT_NONE, True, None)
        mlm_loss = cross_entropy_none(scores, mlm_labels.view(-1)) if mlm_labels is not None else 0
        itm_loss = cross_entropy_none(itm.view(-1, 2), itm_labels.view(-1)) if itm_labels is not None else 0
        return dict(mlm_scores=scores.view(b, lt, v), mlm_loss=mlm_loss, mlm_labels=mlm_labels, itm_scores=itm,
                    itm_loss=itm_loss, itm_labels=itm_labels)
