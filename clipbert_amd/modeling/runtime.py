"""Execution context shared by all modules of one ClipBert instance; dropout seed streams; K split of the weight-gradient GEMMs."""
from typing import Optional

import torch

from .. import ops
from ..params import ParamBank

_HOOK = {"encoder": "after_encoder_backward", "cnn": "after_res5_backward"}


def even_pixel_rows(n, h, w):
    """rows of the (n * h * w)-row image of an (n, h, w) map that hold its even pixels (2i, 2j), in (n, i, j) order"""
    return (torch.arange(n).view(n, 1, 1) * (h * w) + (torch.arange(0, h, 2)).view(1, -1, 1) * w + torch.arange(0, w, 2).view(1, 1, -1)).reshape(-1)


def parity_class_rows(n, h, w):
    """output row map of the 3x3 stride-2 data gradient by parity classes (cb_gemm_desc.dgrad_s2) onto an (n, h, w) map, h and w even:
    class-major, class = 2 * (y & 1) + (x & 1), each class in the (n, y >> 1, x >> 1) order of the compact gradient's pixel table"""
    even = even_pixel_rows(n, h, w)
    return torch.cat([even + py * w + px for py in (0, 1) for px in (0, 1)])


def even_pixel_index(n, h, w):
    """per row of the (n, h, w) map: the row of the compact even-pixel image that holds it, -1 for the other three pixels of each 2 x 2 patch"""
    even = even_pixel_rows(n, h, w)
    t = torch.full((n * h * w,), -1, dtype=torch.int64)
    t[even] = torch.arange(even.numel())
    return t


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
        self.forward_count = 0                           # host counter folded into every dropout seed (and the device-drawn pixel
                                                         # selection's): each forward (each clip of a clip loop) draws its own
                                                         # masks; kept in the saved pack

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

    def rowmap(self, kind, n, h, w, device):
        """cached int32 device copy of even_pixel_rows / parity_class_rows / even_pixel_index (``kind``: the function)"""
        key = (kind.__name__, n, h, w, str(device))
        t = self.rowmaps.get(key)
        if t is None:
            t = self.rowmaps[key] = kind(n, h, w).to(torch.int32).to(device)
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
_SITE_PIXEL = 7          # not a dropout: the pixel sub-sampling drawn on the device (ops.pixel_sample), a seed stream of its own
_SITE_MLM = 8            # not a dropout: the masked-LM token masking drawn on the device (ops.mlm_mask), a seed stream of its own


def _seed(site, layer=0, fwd=0):
    """seed of one dropout site of one layer of the fwd-th forward of this process (the device word *rt.seed_dev is added
    on top by the kernels, so hipGraph replays -- where `fwd` is frozen at capture -- still draw fresh masks)"""
    return ((site * 1000003 + layer * 7919) * 2654435761 + fwd * 0x9E3779B97F4A7C15) % (1 << 62)
