"""Task heads: small autograd nodes (one consumer each, so autograd never has to add tensors), loss nodes, the five task models."""
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..ops import ACT_GELU, ACT_NONE, ACT_RELU, KROW
from .cnn import conv_gather
from .encoder import ClipBertBaseModel, _drop_p, _linear_wgrad
from .modules import BatchNorm1d, Linear, _cfg_get, _make_mlp, _PreTrainingHeads, as_config
from .runtime import _SITE_REG, Runtime, _seed


def _row_gather(rt, operand, rows, k, device):
    """gather block of ``rows`` = (n_seg, seg_len, seg_stride_rows) of a (*, k) matrix: n_seg one-row images of seg_len pixels"""
    nseg, seglen, segstride = rows
    return conv_gather(rt, operand, nseg, 1, seglen, k, 1, 1, 0, device, sN=segstride * k, sH=0)


class _LinearFn(torch.autograd.Function):
    """y = act(x W^T + b).  ``rows`` = (n_seg, seg_len, seg_stride_rows) selects x rows (b*stride + t)."""
    @staticmethod
    def forward(ctx, anchor, x, rt, weight, bias, act, out_f32, rows):
        n, k = weight.shape
        dev = x.device
        x2 = x.reshape(-1, k)
        m = x2.shape[0] if rows is None else rows[0] * rows[1]
        gather = {} if rows is None else _row_gather(rt, "a", rows, k, dev)
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
                           gather=None if rows is None else _row_gather(rt, "b", rows, k, dy.device), defer_bias=True)
        if rows is None:
            dx, rowmap = torch.empty(x2.shape, dtype=dt, device=dy.device), None
        else:                                           # (rows outside the segments get no gradient)
            dx, rowmap = ops.zeros(x2.shape, dt, dy.device), rt.strided_rowmap(rows[0], 1, rows[2], 1, rows[1], 1, dy.device)
        ops.gemm(g, bank.compute(weight), m, k, n, out=dx, lda=g.stride(0), b_mode=KROW, c_rowmap=rowmap)
        if gb is not None:
            ops.colsum(g, gb, m, n)
        return None, dx.view(ctx.x_shape), None, None, None, None, None, None


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

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    def forward(self, text_input_ids, visual_inputs, text_input_mask, mlm_labels=None, itm_labels=None, src_row=None):
        rt = self.rt
        seq, pooled = self.bert(text_input_ids, visual_inputs, text_input_mask, src_row)
        b, L, d = seq.shape
        lt = text_input_mask.shape[1]
        pred = self.cls.predictions
        # heads on the TEXT rows only (modeling.py:283-285): gathered inside the GEMM loader
        h = _LinearFn.apply(rt.anchor, seq, rt, pred.transform.dense.weight, pred.transform.dense.bias, ACT_GELU, False,
                            (b, lt, L))
        h = _LayerNormFn.apply(rt.anchor, h, rt, pred.transform.LayerNorm)
        scores = _LinearFn.apply(rt.anchor, h, rt, pred.decoder.weight, pred.bias, ACT_NONE, True, None)
        rel = self.cls.seq_relationship
        itm = _LinearFn.apply(rt.anchor, pooled, rt, rel.weight, rel.bias, ACT_NONE, True, None)
        v = self.config.vocab_size
        mlm_loss = cross_entropy_none(scores, mlm_labels.view(-1)) if mlm_labels is not None else 0
        itm_loss = cross_entropy_none(itm.view(-1, 2), itm_labels.view(-1)) if itm_labels is not None else 0
        return dict(mlm_scores=scores.view(b, lt, v), mlm_loss=mlm_loss, mlm_labels=mlm_labels, itm_scores=itm,
                    itm_loss=itm_loss, itm_labels=itm_labels)
