"""Execution context shared by all modules of one ClipBert instance; dropout seed streams; K split of the weight-gradient GEMMs."""
from typing import Optional

import torch

from .. import ops
from ..params import ParamBank

_HOOK = {"encoder": "after_encoder_backward", "cnn": "after_res5_backward"}


class Runtime:
    def __init__(self):
        self.bank: Optional[ParamBank] = None
        self.dtype = torch.bfloat16
        self.tables = {}
        self.rowmaps = {}
        self.seed_dev: Optional[torch.Tensor] = None     # device int64 added to every dropout seed
        self.anchor: Optional[torch.Tensor] = None       # requires_grad leaf that keeps the coarse nodes alive
        self.stem_w = None
        self.after_encoder_backward = None               # hook: launch the transformer-bucket all-reduce
        self.pending_encoder_nodes = 0                   # encoder autograd nodes created and not yet run backward: the hook
                                                         # fires when the LAST of them finished (multi-clip loops run several)
        self.after_res5_backward = None                  # hook: every gradient of grid_encoder + res5 is enqueued (fires inside the
                                                         # LAST ResNet backward of a step): their all-reduce can start while res4 / res3 run
        self.pending_cnn_nodes = 0
        self.prepare_args = None                         # keyword arguments of the prepare() call that built this runtime
        self._ln_off = None                              # (bank, offsets of the encoder LayerNorm gradients): cache of _ln_offsets
        self.forward_count = 0                           # host counter folded into every dropout seed: each forward (each
                                                         # clip of a clip loop) draws its own masks; kept in the saved pack

    # ---- step bookkeeping: each hook fires in the LAST pending backward of its kind ("encoder" | "cnn") ---------------------------
    def begin_step(self):
        """a new forward + backward begins: no coarse node of an earlier one counts as pending"""
        self.pending_encoder_nodes = self.pending_cnn_nodes = 0

    def fire_if_last(self, kind, left=1):
        """call the hook of ``kind`` if at most ``left`` of its nodes are pending (1: the one whose backward is running)"""
        hook = getattr(self, _HOOK[kind])
        if hook is not None and getattr(self, f"pending_{kind}_nodes") <= left:
            hook()

    def node_done(self, kind, fire=False):
        """the backward of one node of ``kind`` has been enqueued; ``fire``: its hook follows if that was the last one pending"""
        setattr(self, f"pending_{kind}_nodes", max(0, getattr(self, f"pending_{kind}_nodes") - 1))
        if fire:
            self.fire_if_last(kind, left=0)

    def table(self, n, oh, ow, stride, pad, sN, sH, sW, device):
        key = (n, oh, ow, stride, pad, sN, sH, sW, str(device))
        t = self.tables.get(key)
        if t is None:
            t = ops.build_pixel_table(n, oh, ow, stride, pad, sN, sH, sW, device)
            self.tables[key] = t
        return t

    def strided_rowmap(self, n, h, w, oh, ow, stride, device):
        key = (n, h, w, oh, ow, stride, str(device))
        t = self.rowmaps.get(key)
        if t is None:
            t = (torch.arange(n).view(n, 1, 1) * (h * w) + (torch.arange(oh) * stride).view(1, oh, 1) * w
                 + (torch.arange(ow) * stride).view(1, 1, ow)).reshape(-1).to(torch.int32).to(device)
            self.rowmaps[key] = t
        return t


def _pick_split(mo, no, kred):
    """(split_k, tile) for weight-gradient GEMMs (small outputs, long pixel/token reductions).  Measured on MI355X
    (tools/wgrad_probe2.py): one 64x64 block per CU is latency-bound (~0.3 us per 64-deep K tile), so long reductions
    are split until ~400 blocks are in flight; the partial sums combine through row-coalesced fp32 atomics.  Short
    reductions (transformer weights over 1312 tokens) lose more to the atomics than they gain."""
    ktiles = (kred + 63) // 64
    b64 = ((mo + 63) // 64) * ((no + 63) // 64)
    if b64 >= 200 or ktiles < 64:
        return 1, 0
    split = max(1, min(ktiles // 8, (400 + b64 // 2) // b64))
    return split, 0          # tile 0: cb_gemm's tuned table / heuristics choose the tile (and may refine the split)


# dropout sites -> distinct seed streams
_SITE_EMB, _SITE_ATTN, _SITE_SELF_OUT, _SITE_OUT, _SITE_POOL, _SITE_REG = 1, 2, 3, 4, 5, 6


def _seed(site, layer=0, fwd=0):
    """seed of one dropout site of one layer of the fwd-th forward of this process (the device word *rt.seed_dev is added
    on top by the kernels, so hipGraph replays -- where `fwd` is frozen at capture -- still draw fresh masks)"""
    return ((site * 1000003 + layer * 7919) * 2654435761 + fwd * 0x9E3779B97F4A7C15) % (1 << 62)
