"""End-to-end wrapper: the grid-feature backbone and a task transformer over one runtime and one parameter bank."""
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..params import ParamBank
from .cnn import GridFeatBackbone
from .heads import ClipBertForPreTraining, ClipBertForVideoTextRetrieval
from .modules import Conv2d, FrozenBatchNorm2d, _GridConv, as_config
from .runtime import Runtime


class ClipBert(nn.Module):
    """src/modeling/e2e_model.py:14-50."""
    def __init__(self, config, input_format="BGR", detectron2_model_cfg=None, transformer_cls=ClipBertForPreTraining):
        super().__init__()
        config = as_config(config)
        self.config = config
        self.detectron2_model_cfg = detectron2_model_cfg
        self.cnn = GridFeatBackbone(detectron2_model_cfg=detectron2_model_cfg, config=config, input_format=input_format)
        self.transformer = transformer_cls(config)
        self.retrieval = transformer_cls == ClipBertForVideoTextRetrieval
        self.rt: Optional[Runtime] = None
        self._src_cache = {}
        # nn.Module.load_state_dict copies into the fp32 master views of a prepared model: everything derived from them
        # (bf16 compute copies, folded FrozenBN vectors, packed stem filter) is refreshed afterwards -- also when only
        # a sub-module is loaded (load_state_dict_with_mismatch(model.transformer, ...), load_separate_ckpt)
        # (post-hooks fire for the module load_state_dict was CALLED on only: cnn.feature is what load_detectron2_backbone loads)
        for mod in (self, self.cnn, self.cnn.feature, self.transformer, self.transformer.bert):
            mod.register_load_state_dict_post_hook(lambda _m, _keys, owner=self: owner.refresh_compute())

    def refresh_compute(self):
        if self.rt is None:
            return
        self.rt.bank.sync_compute()
        self.rt.stem_w = None
        for m in self.modules():
            if isinstance(m, Conv2d):
                m._ss = None

    # ---- MI355X runtime --------------------------------------------------------------------------------
    def prepare(self, dtype=torch.bfloat16, device=None, transformer_lr_mul_prefix="", cnn_lr_mul_prefix="grid_encoder", overlap_wgrad=0):
        """Move parameters into the flat HBM buffers and build compute copies.  Call after loading
        weights / changing requires_grad (freeze_cnn_backbone) and before the first forward.  ``overlap_wgrad`` must be 0: the
        weight gradients on concurrent streams were measured slower and removed."""
        if overlap_wgrad:
            raise ValueError(f"prepare(overlap_wgrad={overlap_wgrad!r}): weight gradients on side streams were measured slower "
                             "(profiles/r06a_overlap_ab.txt) and are no longer available; pass 0")
        device = torch.device(device) if device is not None else next(self.parameters()).device
        for buf_owner in self.modules():
            if isinstance(buf_owner, FrozenBatchNorm2d):
                buf_owner.to(device)
        rt = Runtime()
        rt.dtype = dtype
        # re-preparing (freeze_cnn_backbone on a prepared model) must rebuild the SAME parameter-group layout
        rt.prepare_args = dict(dtype=dtype, device=device, transformer_lr_mul_prefix=transformer_lr_mul_prefix,
                               cnn_lr_mul_prefix=cnn_lr_mul_prefix)
        rt.bank = ParamBank(self, device, dtype, transformer_lr_mul_prefix, cnn_lr_mul_prefix)
        rt.seed_dev = torch.zeros(1, dtype=torch.int64, device=device)
        rt.anchor = torch.zeros(1, dtype=torch.float32, device=device, requires_grad=True)
        if dtype == torch.bfloat16 and (device.type == "cuda" or ops._ALLOW_HOST_POINTERS):
            ops.splitk_workspace(device)            # scratch of cb_gemm's K-split: allocated here, before any hipGraph capture
        for m in self.modules():
            if hasattr(m, "rt"):
                m.rt = rt
            if isinstance(m, (Conv2d,)):
                m._ss = None
        enc = []
        for layer in self.transformer.bert.encoder.layer:
            enc += [layer.attention.self.query.weight, layer.attention.self.key.weight, layer.attention.self.value.weight,
                    layer.attention.output.dense.weight, layer.intermediate.dense.weight, layer.output.dense.weight]
        rt.bank.set_lazy_span(enc)
        # the ResNet's trainable convolution weights + the grid encoder's: one weight-gradient launch each per backward -> first-writer stores
        if dtype == torch.bfloat16:
            rt.bank.set_fresh_params([m.weight for m in self.cnn.modules() if isinstance(m, (Conv2d, _GridConv)) and rt.bank.is_trainable(m.weight)])
        return self

    def grid_features(self, visual_inputs):
        """(Bv, T, 3, H, W) frames (tensor or data.RawFrames) -> (Bv, T, H', W', hidden) grid features: the CNN half of forward() on its own, so that
        inference can compute each clip's features once and reuse them across text mini-batches (SURVEY 8f N1;
        the reference recomputes them per mini-batch, run_video_retrieval.py:655-666)."""
        if self.rt is None:
            self.prepare(device=visual_inputs.device)
        return self.cnn(visual_inputs)

    def forward(self, batch):
        vis = batch["visual_inputs"]
        if self.rt is None:
            self.prepare(device=vis.device)
        batch["visual_inputs"] = self.cnn(vis)
        return self.forward_from_grid(batch)

    def forward_from_grid(self, batch, clip_fold: int = 1):
        """forward() for a batch whose ``visual_inputs`` already are grid features (see grid_features).

        clip_fold = n > 1: the grid holds n clips per video, video-major ((Bv*n, T, H', W', d): row v*n + c is clip c of
        video v -- the plain ``view`` of the reference's (B, n*T, 3, H, W) frame tensor, no copy), and the text batch is
        the reference's batch repeated n times, clip-major (row c*B' + j = pair j looking at clip c).  One forward then
        does what the reference's clip loop does in n (run_video_retrieval.py:396-401); logits come back clip-major, i.e.
        ``logits.view(n, B', C)`` is the stack the loop builds with torch.stack."""
        repeat_counts = batch["n_examples_list"]
        del batch["n_examples_list"]
        vis = batch["visual_inputs"]
        # repeat_tensor_rows (data_utils.py:344-357) is fused into the visual-embedding gather
        src_row = None
        if clip_fold > 1:
            src_row = self._src_rows(repeat_counts, clip_fold, vis.device)
            assert vis.shape[0] == len(repeat_counts) * clip_fold, "clip_fold: grid rows != videos x clips"
        elif sum(repeat_counts) != len(repeat_counts):
            src_row = self._src_rows(repeat_counts, 1, vis.device)
        n_txt = batch["text_input_ids"].shape[0]
        if clip_fold > 1 and src_row is not None and n_txt * clip_fold == src_row.numel():
            batch["text_repeat"] = clip_fold           # the captions of ONE clip: every clip reads them in place (no repeated copies)
        elif src_row is not None and src_row.numel() != n_txt:
            raise ValueError(f"n_examples_list describes {src_row.numel()} (video, text) pairs but the text batch has "
                             f"{n_txt} rows")
        if self.retrieval:
            batch["sample_size"] = len(repeat_counts)
        return self.transformer(src_row=src_row, **batch)

    def _src_rows(self, counts, clip_fold, device):
        """grid row of every (video, text) pair, clip-major: pair j of clip c reads row video(j) * clip_fold + c (cached per key)"""
        key = (tuple(counts), clip_fold, str(device))
        src_row = self._src_cache.get(key)
        if src_row is None:
            per_video = [i for i, r in enumerate(counts) for _ in range(r)]
            src_row = torch.tensor([v * clip_fold + c for c in range(clip_fold) for v in per_video], dtype=torch.int32, device=device)
            self._src_cache[key] = src_row
        return src_row

    def load_separate_ckpt(self, cnn_weights_path=None, bert_weights_path=None):
        """e2e_model.py:43-48: detectron2 backbone weights (``grid_feat_R-50.pth`` / a detectron2 ``.pkl`` / a torchvision
        ResNet-50 state dict, see clipbert_amd.checkpoint) into ``cnn.feature`` and a BERT / ClipBERT transformer
        checkpoint into ``transformer``.  Works before or after prepare(); raises if a file matches no key at all."""
        from .. import checkpoint as ckpt
        if cnn_weights_path:
            n = ckpt.load_detectron2_backbone(self.cnn, cnn_weights_path)
            if n == 0:
                raise RuntimeError(f"{cnn_weights_path}: no key of the checkpoint matches the ResNet-50 grid backbone")
        if bert_weights_path:
            n = load_state_dict_with_mismatch(self.transformer, bert_weights_path)
            if n == 0:
                raise RuntimeError(f"{bert_weights_path}: no key of the checkpoint matches {type(self.transformer).__name__}")
        self.refresh_compute()                  # (the load hooks already did it; kept explicit: masters -> compute copies)

    def freeze_cnn_backbone(self):
        """e2e_model.py:49-51.  Changes which parameters are trainable, i.e. the layout of the flat buffers: call it
        before prepare() / before building the optimizer."""
        if self.rt is not None and self.rt.bank.clients > 0:
            raise RuntimeError("freeze_cnn_backbone() after an optimizer / GradSync was built on this model's parameter "
                               "bank: freeze first, then prepare() and build the optimizer")
        for _n, p in self.cnn.feature.named_parameters():
            p.requires_grad = False
        if self.rt is not None:
            self.prepare(**self.rt.prepare_args)


def load_state_dict_with_mismatch(model: nn.Module, loaded_state_dict_or_path) -> int:
    """Key/shape tolerant load (src/utils/load_save.py:71-100): accepts a state dict or a path to one; drops
    shape-mismatched and unknown keys (e.g. the reference checkpoint's dead RPN/ROI-head weights), loads the rest
    non-strictly.  Returns the number of tensors loaded (the reference logs the key differences instead)."""
    sd = loaded_state_dict_or_path
    if isinstance(sd, (str, bytes)) or hasattr(sd, "__fspath__"):
        sd = torch.load(sd, map_location="cpu")
    own = model.state_dict()
    ok = {k: v for k, v in sd.items() if k in own and tuple(own[k].shape) == tuple(v.shape)}
    model.load_state_dict(ok, strict=False)
    return len(ok)
