"""Cross-modal BERT encoder: explicit forward / backward of embeddings, the transformer layers and the pooler."""
from collections import namedtuple
from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch
from torch import nn

from .. import ops
from ..ops import ACT_GELU, ACT_TANH, KROW
from .modules import BertEmbeddings, BertEncoder, BertPooler, VisualInputEmbedding, _cfg_get, as_config
from .runtime import _SITE_ATTN, _SITE_EMB, _SITE_OUT, _SITE_PIXEL, _SITE_POOL, _SITE_SELF_OUT, Runtime, _pick_split, _seed


class ClipBertBaseModel(nn.Module):
    """Embeddings + 12-layer encoder + pooler (src/modeling/modeling.py:156-238)."""
    def __init__(self, config):
        super().__init__()
        config = as_config(config)
        assert _cfg_get(config, "hidden_act", "gelu") == "gelu", "only the exact-erf GELU of base_model.json is implemented"
        assert config.hidden_size // config.num_attention_heads == 64, "attention kernels are built for head size 64"
        self.config = config
        self.embeddings = BertEmbeddings(config)
        self.visual_embeddings = VisualInputEmbedding(config)
        self.encoder = BertEncoder(config)
        self.pooler = BertPooler(config)
        self.rt: Optional[Runtime] = None

    def get_input_embeddings(self):
        return self.embeddings.word_embeddings

    def forward(self, text_input_ids, visual_inputs, attention_mask, src_row=None, pooled_dropout=False, text_repeat=1):
        """visual_inputs: grid (Bv, n_frm, H', W', d); src_row maps each text row to its grid row
        (the fused form of repeat_tensor_rows).  Returns (sequence_output (B, L, d), pooled (B, d)).
        text_repeat = n: the (P, Lt) text batch stands for n*P rows (row b = text row b % P: the captions of a folded clip loop,
        read in place by the embedding kernels instead of from n repeated copies)."""
        seq, pooled = _EncoderFn.apply(self.rt.anchor, visual_inputs, self, text_input_ids, attention_mask, src_row,
                                       pooled_dropout, text_repeat)
        b = text_input_ids.shape[0] * text_repeat
        return seq.view(b, -1, self.config.hidden_size), pooled


# what one encoder layer keeps for its backward (its GEMM inputs x, a, hact live in the layer-stacked buffers of the pack)
_LayerSaved = namedtuple("_LayerSaved", "qkv ctx lse a_pre mean1 rstd1 hsave o_pre mean2 rstd2")


def _drop_p(model, training, key="hidden_dropout_prob"):
    return float(_cfg_get(model.config, key, 0.0)) if training else 0.0


def encoder_forward(model: ClipBertBaseModel, grid, ids, mask, src_row, pooled_dropout, save, text_repeat=1):
    rt, cfg = model.rt, model.config
    bank, dt, dev = rt.bank, rt.dtype, ids.device
    d, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    training = model.training
    p_h = _drop_p(model, training)
    p_a = _drop_p(model, training, "attention_probs_dropout_prob")
    bsz, lt = ids.shape[0] * text_repeat, ids.shape[1]
    bv, t, hg, wg, _ = grid.shape
    lv = hg * wg
    nsamp = int(_cfg_get(cfg, "pixel_random_sampling_size", 0) or 0)
    sampling = _cfg_get(cfg, "pixel_sampling", "host") or "host"
    if sampling not in ("host", "device"):
        raise ValueError(f"pixel_sampling must be 'host' or 'device', not {sampling!r}")
    sample = nsamp > 0 and training and nsamp < lv
    fwd_i = 0
    if p_h > 0 or p_a > 0 or (sample and sampling == "device"):
        fwd_i = rt.forward_count              # every training forward draws its own dropout masks (the reference's nn.Dropout does) and
        rt.forward_count += 1                 # its own device-side pixel selection; the backward regenerates the masks from pack.fwd_i
    # optional random pixel sub-sampling: training phase of pre-training only (modeling.py:80-88)
    sel = None
    if sample:
        if sampling == "device":              # one launch, seeded like a dropout site: capturable, fresh per replay (cb_pixel_sample)
            sel = ops.pixel_sample(lv, nsamp, _seed(_SITE_PIXEL, 0, fwd_i), rt.seed_dev, device=dev)
        else:
            idx = np.sort(np.random.choice(lv, size=nsamp, replace=False))     # numpy global RNG, as the reference
            sel = torch.from_numpy(idx.astype(np.int32)).to(dev)
        lv = nsamp
    L = lt + lv
    M = bsz * L
    if src_row is None:
        assert bv == bsz, "visual batch and text batch differ: pass src_row (n_examples_list)"
    key_mask = torch.empty(bsz, L, dtype=torch.float32, device=dev)        # filled by the two embedding kernels
    mask_c = mask if (mask.dtype == torch.int64 and mask.is_contiguous()) else mask.to(torch.int64).contiguous()
    nl, ff = len(model.encoder.layer), cfg.intermediate_size
    # The operands of the weight-gradient GEMMs are kept LAYER-STACKED ([layer, M, *]): the backward then computes the
    # weight gradients of all layers of one kind in a single strided-batched launch (encoder_backward).
    stk = None
    if save:
        stk = SimpleNamespace(x=torch.empty(nl, M, d, dtype=dt, device=dev), ctx=torch.empty(nl, M, d, dtype=dt, device=dev),
                              a=torch.empty(nl, M, d, dtype=dt, device=dev), hact=torch.empty(nl, M, ff, dtype=dt, device=dev))
    x = stk.x[0] if save else torch.empty(M, d, dtype=dt, device=dev)
    pre = torch.empty(M, d, dtype=dt, device=dev) if save else None
    mean0, rstd0 = torch.empty(2, M, dtype=torch.float32, device=dev) if save else (None, None)
    emb, vemb = model.embeddings, model.visual_embeddings
    ids_c = ids.contiguous()
    ops.text_embed_fwd(ids_c, bank.compute(emb.word_embeddings.weight), bank.compute(emb.position_embeddings.weight),
                       bank.compute(emb.token_type_embeddings.weight)[0], emb.LayerNorm.weight, emb.LayerNorm.bias, x, pre,
                       mean0, rstd0, lt, L, eps, attn_mask=mask_c, key_mask=key_mask, repeat=text_repeat)
    grid_c = grid.contiguous()
    ops.visual_embed_fwd(grid_c, src_row, sel, bank.compute(vemb.row_position_embeddings.weight),
                         bank.compute(vemb.col_position_embeddings.weight), bank.compute(vemb.token_type_embeddings.weight)[0],
                         vemb.LayerNorm.weight, vemb.LayerNorm.bias, x, pre, mean0, rstd0, bsz, lv, lt, L, eps, key_mask=key_mask)
    if p_h > 0:
        ops.dropout(x, p_h, _seed(_SITE_EMB, 0, fwd_i), rt.seed_dev, out=x)
    layers = []
    for li, layer in enumerate(model.encoder.layer):
        att, so, it, ou = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
        wqkv = bank.compute_span(att.query.weight, att.value.weight, (3 * d, d))
        bqkv = bank.master_span(att.query.bias, att.value.bias, (3 * d,))
        qkv = torch.empty(M, 3 * d, dtype=dt, device=dev)
        ops.gemm(x, wqkv, M, 3 * d, d, out=qkv, shift=bqkv)
        ctx, lse = ops.attention_fwd(qkv, key_mask, bsz, L, nh, save_lse=save, dropout_p=p_a,
                                     dropout_seed=_seed(_SITE_ATTN, li, fwd_i), seed_ptr=rt.seed_dev, out=stk.ctx[li] if save else None)
        a_pre = torch.empty(M, d, dtype=dt, device=dev)
        ops.gemm(ctx, bank.compute(so.dense.weight), M, d, d, out=a_pre, shift=so.dense.bias, residual=x, dropout_p=p_h,
                 dropout_seed=_seed(_SITE_SELF_OUT, li, fwd_i), seed_ptr=rt.seed_dev)
        a, mean1, rstd1 = ops.layernorm_fwd(a_pre, so.LayerNorm.weight, so.LayerNorm.bias, eps, save_stats=save,
                                            out=stk.a[li] if save else None)
        hact = stk.hact[li] if save else torch.empty(M, ff, dtype=dt, device=dev)
        hsave = torch.empty(M, ff, dtype=dt, device=dev) if save else None     # gelu'(pre), for the backward
        # (training: the second output is gelu'(pre-activation), all the backward needs of it -- one evaluation of exp / erfc for both, and
        # the FFN2 data-gradient epilogue multiplies by the stored value instead of evaluating the derivative: CB_ACT_GELU_SAVE_GRAD)
        ops.gemm(a, bank.compute(it.dense.weight), M, ff, d, out=hact, shift=it.dense.bias,
                 act=ops.ACT_GELU_SAVE_GRAD if save else ACT_GELU, out2=hsave)
        o_pre = torch.empty(M, d, dtype=dt, device=dev)
        ops.gemm(hact, bank.compute(ou.dense.weight), M, d, ff, out=o_pre, shift=ou.dense.bias, residual=a, dropout_p=p_h,
                 dropout_seed=_seed(_SITE_OUT, li, fwd_i), seed_ptr=rt.seed_dev)
        out, mean2, rstd2 = ops.layernorm_fwd(o_pre, ou.LayerNorm.weight, ou.LayerNorm.bias, eps, save_stats=save,
                                              out=stk.x[li + 1] if (save and li + 1 < nl) else None)
        if save:
            layers.append(_LayerSaved(qkv, ctx, lse, a_pre, mean1, rstd1, hsave, o_pre, mean2, rstd2))
        x = out
    pooled = torch.empty(bsz, d, dtype=dt, device=dev)
    p_pool = p_h if pooled_dropout else 0.0
    pooled_raw = torch.empty(bsz, d, dtype=dt, device=dev) if (save and p_pool > 0) else None
    pw = model.pooler.dense
    # the pooler's dropout rides on the GEMM epilogue, unless the backward needs tanh's output from before it: then it is a launch of its own
    drop = dict(dropout_p=p_pool, dropout_seed=_seed(_SITE_POOL, 0, fwd_i), seed_ptr=rt.seed_dev) if pooled_raw is None else {}
    ops.gemm(x, bank.compute(pw.weight), bsz, d, d, out=pooled if pooled_raw is None else pooled_raw, lda=L * d, shift=pw.bias, act=ACT_TANH, **drop)
    if pooled_raw is not None:
        ops.dropout(pooled_raw, p_pool, _seed(_SITE_POOL, 0, fwd_i), rt.seed_dev, out=pooled)
    pack = None
    if save:
        pack = SimpleNamespace(layers=layers, x_final=x, pooled=pooled, pooled_raw=pooled_raw, p_pool=p_pool, pre=pre,
                               mean0=mean0, rstd0=rstd0, ids=ids_c, key_mask=key_mask, src_row=src_row, sel=sel, bsz=bsz,
                               lt=lt, lv=lv, L=L, grid_shape=tuple(grid.shape), p_h=p_h, p_a=p_a, stk=stk, fwd_i=fwd_i, text_repeat=text_repeat)
    return x, pooled, pack


def _linear_wgrad(g, x, m, n, k, gw, gb, ldx=None, gather=None, defer_bias=False):
    """dW[n,k] += g[m,n]^T x[m,k] into the gradient image ``gw`` and db[n] += colsum(g) into ``gb`` (None: frozen).  The bias rides on
    the weight-gradient launch (row sums of g on the matrix core, cb_gemm_desc.a_rowsum) unless the weight is frozen or x's rows are
    gathered (``gather``: the operand-"b" block of cnn.conv_gather); then ops.colsum does it -- here, or with ``defer_bias`` in the
    caller's own time: the image still owed is returned."""
    rides = gw is not None and gather is None
    if gw is not None:
        split, tile = _pick_split(n, k, m)
        xkw = gather if gather is not None else dict(b_mode=KROW, ldb=ldx if ldx is not None else x.stride(0), a_rowsum=gb)
        ops.gemm(g, x, n, k, m, out=gw, a_mode=KROW, lda=g.stride(0), **xkw, accumulate=True, split_k=split, tile=tile)
    owed = None if rides else gb
    if owed is not None and not defer_bias:
        ops.colsum(g, owed, m, n)
        owed = None
    return owed


def _uniform_stride(tensors):
    """element stride between consecutive tensors of a list if they are equally spaced views of one buffer, else None"""
    if any(t is None for t in tensors):
        return None
    if len(tensors) == 1:
        return 0
    steps = {b.data_ptr() - a.data_ptr() for a, b in zip(tensors, tensors[1:])}
    step, esz = steps.pop(), tensors[0].element_size()
    return step // esz if (not steps and step > 0 and step % esz == 0) else None


def _encoder_wgrads(model, pk, gs, M):
    """Weight and bias gradients of every encoder layer: one strided-batched weight-gradient GEMM per kind when the
    layers' gradient images are equally spaced in the flat gradient buffer (they are: same parameter order in every
    layer), per-layer launches otherwise (frozen layers)."""
    rt, cfg = model.rt, model.config
    bank = rt.bank
    d, ff = cfg.hidden_size, cfg.intermediate_size
    layers = list(model.encoder.layer)
    nl, stk = len(layers), pk.stk

    def qkv(l, name, shape):
        q, v = getattr(l.attention.self.query, name), getattr(l.attention.self.value, name)
        return bank.grad_span(q, v, shape) if bank.is_trainable(q) else None

    def imgs(lin):
        return [bank.grad_image(lin(l).weight) for l in layers], [bank.grad_image(lin(l).bias) for l in layers]

    kinds = [  # (upstream gradient stack, input stack, out features, in features, (dW images, db images), name of the kind)
        (gs.out, stk.hact, d, ff, imgs(lambda l: l.output.dense), "out"),
        (gs.hp, stk.a, ff, d, imgs(lambda l: l.intermediate.dense), "ffn"),
        (gs.att, stk.ctx, d, d, imgs(lambda l: l.attention.output.dense), "att"),
        (gs.qkv, stk.x, 3 * d, d, ([qkv(l, "weight", (3 * d, d)) for l in layers], [qkv(l, "bias", (3 * d,)) for l in layers]), "qkv"),
    ]
    def batch_strides(n, k, gws, gbs):
        """(dW stride, db stride) between consecutive layers, or None where the kind cannot run as one strided-batched launch"""
        st = (_uniform_stride(gws), _uniform_stride(gbs))
        return st if (None not in st and n % 8 == 0 and k % 8 == 0) else None

    strides = [batch_strides(n, k, *im) for _g, _x, n, k, im, _kd in kinds]
    all_batched = None not in strides
    # first-writer stores: after zero_grad(lazy=True) the encoder weight gradients were NOT zeroed -- the batched launches
    # overwrite them (no memset, no fp32 read-modify-write); any other path zeroes the span first
    fresh = bank.take_fresh()
    if fresh and not all_batched:
        a, b = bank.lazy_span
        bank.grad[a:b].zero_()
        fresh = False
    if not fresh:
        bank.fold_invalidate()                       # (a second backward of the step accumulates: the first one's norm shares are void)
    bf16 = rt.dtype == torch.bfloat16
    # bf16, every kind batched: all four in ONE grouped launch (cb_gemm_group's row-sum / strided-batch class): 48 problems' 5184 tiles of
    # 128x128 share a grid, so only one last wave of tiles runs on a part-filled chip instead of four (profiles/r06k_enc_wgrad_group_ab.txt).
    # Otherwise one launch per kind, cb_gemm choosing the tile.
    group = [] if (all_batched and bf16) else None
    for (g, x, n, k, (gws, gbs), kind), st in zip(kinds, strides):
        if st is None:
            for li in range(nl):
                _linear_wgrad(g[li], x[li], M, n, k, gws[li], gbs[li])
            continue
        slots = bank.fold_take(ops.sq_slot_count(n, k, nl), "enc:" + kind) if (fresh and bf16) else None
        desc = dict(out=gws[0], a_mode=KROW, lda=n, b_mode=KROW, ldb=k, ldc=k, accumulate=not fresh, a_rowsum=gbs[0], batch=nl,
                    batch_strides=(M * n, M * k, *st), sq_slots=slots)
        if group is None:
            ops.gemm(g, x, n, k, M, **desc)
        else:
            group.append(ops.gemm_desc(g, x, n, k, M, tile=4, **desc))
    if group:
        ops.gemm_group(group, gs.out)


def _ln_offsets(model, dev):
    """(2, 2*n_layers) int64 device tensor: element offsets of the encoder LayerNorms' (weight | bias) gradients in bank.grad, in
    the slot order encoder_backward uses (2*l: attention.output.LayerNorm, 2*l+1: output.LayerNorm); None if any is frozen."""
    rt = model.rt
    cached = rt._ln_off
    if cached is not None and cached[0] is rt.bank:
        return cached[1]
    bank, offs = rt.bank, ([], [])
    for layer in model.encoder.layer:
        for ln in (layer.attention.output.LayerNorm, layer.output.LayerNorm):
            gw, gb = bank.grad_image(ln.weight), bank.grad_image(ln.bias)
            if gw is None or gb is None:
                rt._ln_off = (bank, None)
                return None
            offs[0].append((gw.data_ptr() - bank.grad.data_ptr()) // 4)
            offs[1].append((gb.data_ptr() - bank.grad.data_ptr()) // 4)
    t = torch.tensor(offs, dtype=torch.int64).to(dev)
    rt._ln_off = (bank, t)
    return t


def encoder_backward(model: ClipBertBaseModel, pk, d_seq, d_pooled):
    rt, cfg = model.rt, model.config
    bank, dt = rt.bank, rt.dtype
    d, nh, ff = cfg.hidden_size, cfg.num_attention_heads, cfg.intermediate_size
    bsz, L, lt, lv = pk.bsz, pk.L, pk.lt, pk.lv
    M = bsz * L
    dev = pk.x_final.device
    # ---- pooler ------------------------------------------------------------------------------------
    if d_seq is None:
        dx = ops.zeros((M, d), dt, dev)
    else:
        dx = d_seq.reshape(M, d)
        if dx.dtype != dt or not dx.is_contiguous():
            dx = ops.cast(dx.contiguous(), torch.empty(M, d, dtype=dt, device=dev))
    if d_pooled is not None:
        g = d_pooled.to(dt).contiguous()
        if pk.pooled_raw is not None:
            g = ops.dropout(g, pk.p_pool, _seed(_SITE_POOL, 0, pk.fwd_i), rt.seed_dev)
            g = ops.act_bwd(ACT_TANH, g, pk.pooled_raw)
        else:
            g = ops.act_bwd(ACT_TANH, g, pk.pooled)
        pw = model.pooler.dense
        _linear_wgrad(g, pk.x_final, bsz, d, d, bank.grad_image(pw.weight), bank.grad_image(pw.bias), ldx=L * d)
        ops.gemm(g, bank.compute(pw.weight), bsz, d, d, out=dx, b_mode=KROW, ldc=L * d, accumulate=True)
    # ---- encoder layers, last to first -----------------------------------------------------------------
    # The dgrad chain runs layer by layer; the upstream gradients that the weight gradients need are written into
    # layer-stacked buffers and ALL layers' weight (+ bias) gradients of one kind follow in one strided-batched GEMM
    # each (4 launches instead of 4 per layer: 12x the blocks per launch, 128x128 tiles, no launch tails).
    nl, stk = len(pk.layers), pk.stk
    # LayerNorm parameter gradients: every LN backward stores per-block partial sums (no atomics); ONE launch after the layer
    # loop adds all 2*nl of them onto the gradient buffer in a fixed order (deterministic).  Frozen LN parameters -> atomics path.
    ln_off = _ln_offsets(model, dev)
    nb = ops.ln_part_blocks(M)
    ln_part = torch.empty(2 * nl, nb, 2, d, dtype=torch.float32, device=dev) if ln_off is not None else None

    def ln_bwd(slot, dy, xpre, ln, mean, rstd, seed, g_out):
        """-> (d(pre-LN sum), g = the gradient of the GEMM output under its dropout, written into the weight-gradient stack row g_out)"""
        keep = dict(dx2=g_out) if pk.p_h > 0 else dict(dx=g_out)
        if ln_part is not None:
            d_pre, d_drop = ops.layernorm_bwd_part(dy, xpre, ln.weight, mean, rstd, ln_part[slot], pk.p_h, seed, rt.seed_dev, **keep)
        else:
            d_pre, d_drop = ops.layernorm_bwd(dy, xpre, ln.weight, mean, rstd, bank.grad_image(ln.weight), bank.grad_image(ln.bias), pk.p_h,
                                              seed, rt.seed_dev, **keep)
        return d_pre, d_drop if d_drop is not None else d_pre

    gs = SimpleNamespace(out=torch.empty(nl, M, d, dtype=dt, device=dev), hp=torch.empty(nl, M, ff, dtype=dt, device=dev),
                         att=torch.empty(nl, M, d, dtype=dt, device=dev), qkv=torch.empty(nl, M, 3 * d, dtype=dt, device=dev))
    for li in range(nl - 1, -1, -1):
        layer = model.encoder.layer[li]
        att, so, it, ou = layer.attention.self, layer.attention.output, layer.intermediate, layer.output
        sv = pk.layers[li]
        d_o_pre, g = ln_bwd(2 * li + 1, dx, sv.o_pre, ou.LayerNorm, sv.mean2, sv.rstd2, _seed(_SITE_OUT, li, pk.fwd_i), gs.out[li])
        dhp = gs.hp[li]
        ops.gemm(g, bank.compute(ou.dense.weight), M, ff, d, out=dhp, b_mode=KROW, gelu_grad_pre=sv.hsave,      # dgrad x the stored GELU'
                 act=ops.ACT_SAVED_GRAD)
        da = torch.empty(M, d, dtype=dt, device=dev)
        ops.gemm(dhp, bank.compute(it.dense.weight), M, d, ff, out=da, b_mode=KROW, residual=d_o_pre)
        d_a_pre, g = ln_bwd(2 * li, da, sv.a_pre, so.LayerNorm, sv.mean1, sv.rstd1, _seed(_SITE_SELF_OUT, li, pk.fwd_i), gs.att[li])
        dctx = torch.empty(M, d, dtype=dt, device=dev)
        ops.gemm(g, bank.compute(so.dense.weight), M, d, d, out=dctx, b_mode=KROW)
        dqkv = ops.attention_bwd(sv.qkv, pk.key_mask, sv.ctx, dctx, sv.lse, bsz, L, nh, pk.p_a, _seed(_SITE_ATTN, li, pk.fwd_i), rt.seed_dev,
                                 out=gs.qkv[li])
        wqkv = bank.compute_span(att.query.weight, att.value.weight, (3 * d, d))
        dx = torch.empty(M, d, dtype=dt, device=dev)
        ops.gemm(dqkv, wqkv, M, d, 3 * d, out=dx, b_mode=KROW, residual=d_a_pre)
    if ln_part is not None:
        ops.ln_partials_reduce(ln_part, bank.grad, ln_off[0], ln_off[1])
    _encoder_wgrads(model, pk, gs, M)
    # ---- embeddings -----------------------------------------------------------------------------------
    if pk.p_h > 0:
        dx = ops.dropout(dx, pk.p_h, _seed(_SITE_EMB, 0, pk.fwd_i), rt.seed_dev)
    emb, vemb = model.embeddings, model.visual_embeddings
    dpre = torch.empty(M, d, dtype=dt, device=dev)
    ops.layernorm_bwd(dx, pk.pre, emb.LayerNorm.weight, pk.mean0, pk.rstd0, bank.grad_image(emb.LayerNorm.weight),
                      bank.grad_image(emb.LayerNorm.bias), dx=dpre, rows=bsz * lt, seg=(lt, L, 0))
    ops.layernorm_bwd(dx, pk.pre, vemb.LayerNorm.weight, pk.mean0, pk.rstd0, bank.grad_image(vemb.LayerNorm.weight),
                      bank.grad_image(vemb.LayerNorm.bias), dx=dpre, rows=bsz * lv, seg=(lv, L, lt))
    we = emb.word_embeddings
    ops.text_embed_bwd(dpre, pk.ids, bank.grad_image(we.weight), bank.grad_image(emb.position_embeddings.weight),
                       bank.grad_image(emb.token_type_embeddings.weight)[0], lt, L,
                       we.padding_idx if we.padding_idx is not None else -1, repeat=pk.text_repeat)
    dgrid = ops.zeros(pk.grid_shape, torch.float32, dev)
    ops.visual_embed_bwd(dpre, pk.src_row, pk.sel, dgrid, bank.grad_image(vemb.row_position_embeddings.weight),
                         bank.grad_image(vemb.col_position_embeddings.weight), bank.grad_image(vemb.token_type_embeddings.weight)[0],
                         bsz, lv, lt, L)
    return dgrid if dt == torch.float32 else ops.cast(dgrid, torch.empty(pk.grid_shape, dtype=dt, device=dev))


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, grid, model, ids, mask, src_row, pooled_dropout, text_repeat=1):
        save = ctx.needs_input_grad[0]
        ctx.set_materialize_grads(False)
        seq, pooled, pack = encoder_forward(model, grid, ids, mask, src_row, pooled_dropout, save, text_repeat)
        ctx.model, ctx.pack = model, pack
        if save:
            model.rt.pending_encoder_nodes += 1
        return seq, pooled

    @staticmethod
    def backward(ctx, d_seq, d_pooled):
        dgrid = encoder_backward(ctx.model, ctx.pack, d_seq, d_pooled)
        ctx.pack = None
        # a clip LOOP (train_n_clips forwards before one backward) runs several encoder backwards per step: the
        # transformer gradients are complete -- and may start their all-reduce -- only after the last of them
        ctx.model.rt.node_done("encoder", fire=True)
        return None, dgrid, None, None, None, None, None, None
