"""CNN trunk: explicit forward / backward of the ResNet-50 grid-feature backbone and the grid encoder."""
from typing import Optional

import torch
from torch import nn

from .. import ops
from ..data import RawFrames
from ..ops import ACT_NONE, ACT_RELU, KROW, KROW_GATHER, KROW_TAPS, ROWK_GATHER
from .modules import RESNET50_STAGES, BottleneckBlock, Conv2d, _Detectron2Model, _GridConv, as_config
from .runtime import Runtime, _pick_split, even_pixel_index, even_pixel_rows, parity_class_rows


def _out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def conv_gather(rt: Runtime, operand, n, h, w, c, k, stride, pad, device, out_hw=None, taps=None, sN=None, sH=None):
    """Convolution-as-GEMM geometry of an (n, h, w, c) image under a k x k window: the keyword block of ops.gemm that makes
    ``operand`` the gathered windows, pixel table of the output positions included -- "a": the rows of A (ROWK_GATHER), "b": B, along
    K (KROW_GATHER, weight gradients).  Overrides for what is not a plain NHWC convolution: ``out_hw`` (output size), ``taps`` =
    (R, S, Cin) of the window as the loader walks it, ``sN`` / ``sH`` (element strides of an image / an image row)."""
    oh, ow = out_hw or _out_hw(h, w, k, stride, pad)
    sN, sH = h * w * c if sN is None else sN, w * c if sH is None else sH
    R, S, cin = taps or (k, k, c)
    tab = rt.table(n, oh, ow, stride, pad, sN, sH, c, device)
    kw = dict(R=R, S=S, Cin=cin, H=h, W=w, sH=sH, sW=c)
    kw.update(dict(a_mode=ROWK_GATHER, a_tab=tab, lda=0) if operand == "a" else dict(b_mode=KROW_GATHER, b_tab=tab, ldb=0))
    return kw


class _ConvAs:
    """A convolution of the model run at another stride -- same weight, FrozenBN and window.  Stride 2 -> 1: the 1x1 stride-2 convolutions
    of a stage's first block on an input that holds the even pixels only (they are plain products there).  Stride 1 -> 2: the 3x3
    convolution of a tail block, whose output is read at the even pixels only."""
    def __init__(self, conv, stride):
        self.conv, self.stride = conv, stride

    def __getattr__(self, name):
        return getattr(self.conv, name)


def _conv_fwd(rt: Runtime, x, conv, act=ACT_NONE, residual=None, relu_after=False, res_rowmap=None):
    """``res_rowmap``: the residual is a tensor of other rows, read through this map (output row -> residual row)"""
    n, h, w, cin = x.shape
    k, s, p = conv.k, conv.stride, conv.pad
    oh, ow = _out_hw(h, w, k, s, p)
    cout = conv.cout
    m = n * oh * ow
    y = torch.empty(n, oh, ow, cout, dtype=x.dtype, device=x.device)
    wk = rt.bank.compute(conv.weight).view(cout, k * k * cin)
    scale, shift = conv.scale_shift()
    res2d = residual.view(-1, cout) if residual is not None else None
    plain = k == 1 and s == 1                          # the image itself is the (m, cin) operand
    gather = {} if plain else conv_gather(rt, "a", n, h, w, cin, k, s, p, x.device)
    ops.gemm(x.view(m, cin) if plain else x, wk, m, cout, k * k * cin, out=y.view(m, cout), ldb=k * k * cin, **gather, scale=scale, shift=shift,
             act=act, residual=res2d, relu_after=relu_after, res_rowmap=res_rowmap)
    return y


def _conv_dgrad(rt: Runtime, g, conv, in_shape, scale=None, mask=None, residual=None, out=None, accumulate=False, fuse=None, res_rowmap=None):
    """d(input) of a convolution given g = d(conv output) (already multiplied by the FrozenBN scale).
    Epilogue options: per-channel ``scale`` and ReLU ``mask`` of the PRODUCER of the input, ``residual``.
    ``fuse = (y, s_a, s_b)``: the input is the output y of a ResNet block; the launch also does that block's ReLU x
    FrozenBN-scale backward and returns (t*s_a, t*s_b) with t = d(input) where y > 0 (s_b None -> t itself).
    ``res_rowmap``: the residual exists at some input pixels only (input row -> its row, or -1).
    A 3x3 stride-2 convolution (the tail form's conv2) takes the one-launch parity-class form, cb_gemm_desc.dgrad_s2."""
    n, h, w, cin = in_shape
    _, oh, ow, cout = g.shape
    k, s, p = conv.k, conv.stride, conv.pad
    wk = rt.bank.compute(conv.weight).view(cout, k * k * cin)
    mi = n * h * w
    # stride-2 1x1 convolution: only the even pixels receive a gradient.  When the 2x2 patches tile the input exactly the launch
    # itself writes the zeros of the other three pixels (zero_fill_pitch); otherwise the output is pre-zeroed
    zfill = w if (k == 1 and s == 2 and h % 2 == 0 and w % 2 == 0 and cin % 8 == 0) else 0
    alloc = torch.zeros if (k == 1 and s > 1 and not zfill) else torch.empty       # (the 3x3 stride-2 form writes every input pixel)
    if out is None:
        out = alloc(n, h, w, cin, dtype=g.dtype, device=g.device)
    o2 = out.view(mi, cin)
    r2 = residual.view(-1, cin) if residual is not None else None
    k2 = mask.view(mi, cin) if mask is not None else None
    extra = {}
    second = None
    if fuse is not None:
        assert mask is None and scale is None
        y, s_a, s_b = fuse
        second = alloc(n, h, w, cin, dtype=g.dtype, device=g.device)
        k2 = y.view(mi, cin)
        extra = dict(relu_bwd=True, post_scale=s_a, post_scale2=s_b, out2=second.view(mi, cin))
    if k == 1:
        rowmap = rt.strided_rowmap(n, h, w, oh, ow, s, g.device) if s > 1 else None
        ops.gemm(g.view(n * oh * ow, cout), wk, n * oh * ow, cin, cout, out=o2, b_mode=KROW_TAPS, ldb=cin, R=1, S=1,
                 Cin=cout, c_rowmap=rowmap, scale=scale, mask=k2, residual=r2, accumulate=accumulate, zero_fill_pitch=zfill if s > 1 else 0,
                 res_rowmap=res_rowmap, **extra)
    elif s == 2:
        assert k == 3 and p == 1 and h == 2 * oh and w == 2 * ow and residual is None and fuse is None and not accumulate
        # the windows of the compact g that meet each parity class of input pixels are dense: its stride-1 pad-0 table serves all four
        ops.gemm(g, wk, mi, cin, 9 * cout, out=o2, b_mode=KROW_TAPS, ldb=9 * cin, dgrad_s2=True,
                 **conv_gather(rt, "a", n, oh, ow, cout, 3, 1, 0, g.device, out_hw=(oh, ow)), c_rowmap=rt.rowmap(parity_class_rows, n, h, w, g.device),
                 scale=scale, mask=k2)
    else:
        assert s == 1
        # (the transposed convolution: the k x k windows of g under padding k - 1 - p, taps flipped)
        ops.gemm(g, wk, mi, cin, k * k * cout, out=o2, b_mode=KROW_TAPS, ldb=k * k * cin, flip_taps=True,
                 **conv_gather(rt, "a", n, oh, ow, cout, k, 1, k - 1 - p, g.device), scale=scale, mask=k2, residual=r2,
                 accumulate=accumulate, **extra)
    return (out, second) if fuse is not None else out


def _conv_wgrad(rt: Runtime, g, x, conv, pending=None):
    """dW[co][(r,s,c)] += sum_pixels g[m,co] * x[pix(m,r,s), c], straight into the flat fp32 grad buffer.
    ``pending`` (a list): the launch is only DESCRIBED and appended -- the caller hands the weight gradients of a whole ResNet stage
    to cb_gemm_group at once (they are off the data-gradient chain: a few launches that fill the chip instead of one per convolution)."""
    gw = rt.bank.grad_image(conv.weight)
    if gw is None:
        return
    n, h, w, cin = x.shape
    _, oh, ow, cout = g.shape
    k, s, p = conv.k, conv.stride, conv.pad
    m = n * oh * ow
    kk = k * k * cin
    split, tile = _pick_split(cout, kk, m)
    # first writer of this step (ParamBank.set_fresh_params: the range was not zeroed): the launch STORES (no read-modify-write of the
    # gradient) and leaves its share of the squared norm; a second backward of the step accumulates as before and voids the shares
    bank = rt.bank
    acc, slots = True, None
    if bank.take_fresh_param(conv.weight):
        if rt.dtype == torch.bfloat16 and kk % 8 == 0:
            acc = 2
            slots = bank.fold_take(ops.sq_slot_count(cout, kk), "cnn")
        else:
            ops.zero_(gw)                            # (a form the first-writer store does not cover: zero now, accumulate as ever)
    else:
        bank.fold_invalidate()
    run = ops.gemm if pending is None else (lambda *a, **kw: pending.append(ops.gemm_desc(*a, **kw)))
    plain = k == 1 and s == 1
    xkw = dict(b_mode=KROW, ldb=cin) if plain else conv_gather(rt, "b", n, h, w, cin, k, s, p, x.device)
    run(g.view(m, cout), x.view(m, cin) if plain else x, cout, kk, m, out=gw.view(cout, kk), a_mode=KROW, lda=cout, **xkw, accumulate=acc,
        split_k=split, tile=tile, sq_slots=slots)


def _stem_weight(rt: Runtime, conv: Conv2d):
    """[64][7 rows][8 taps x 4 ch] image of the 7x7x3 stem filter (tap 7 and channel 3 are zero)."""
    if rt.stem_w is None:
        w = conv.weight.detach().float()                         # (64, 3, 7, 7)
        wp = torch.zeros(64, 7, 8, 4, dtype=torch.float32, device=w.device)
        wp[:, :, :7, :3] = w.permute(0, 2, 3, 1)
        rt.stem_w = wp.view(64, 224).to(rt.dtype).contiguous()
    return rt.stem_w


def _block_trainable(rt: Runtime, blk: BottleneckBlock) -> bool:
    return any(rt.bank.is_trainable(c.weight) for c in (blk.conv1, blk.conv2, blk.conv3) + ((blk.shortcut,) if blk.shortcut is not None else ()))


def _res2_block_fused(rt: Runtime, x, blk: BottleneckBlock):
    """one res2 block through cb_res2_block (conv1 -> conv2 -> conv3 + shortcut in ONE launch; forward only)"""
    w = lambda conv: rt.bank.compute(conv.weight)
    sc = blk.shortcut
    return ops.res2_block(x, w(blk.conv1), w(blk.conv2), w(blk.conv3), blk.conv1.scale_shift(), blk.conv2.scale_shift(), blk.conv3.scale_shift(),
                          wsc=w(sc) if sc is not None else None, sssc=sc.scale_shift() if sc is not None else None)


def _res2_fusable(rt: Runtime, x, blk: BottleneckBlock, save: bool) -> bool:
    """the fused forward kernel covers the frozen 64-mid-channel, stride-1 blocks in bf16 (FREEZE_AT = 2: nothing of res2 is saved for a
    backward)"""
    if rt.dtype != torch.bfloat16:
        return False
    if save and _block_trainable(rt, blk):
        return False
    c1, c2, c3 = blk.conv1, blk.conv2, blk.conv3
    return (c1.cout == 64 and c2.cin == 64 and c2.cout == 64 and c3.cout == 256 and c1.stride == 1 and c1.k == 1 and c2.k == 3 and c2.stride == 1
            and c3.k == 1 and c1.cin in (64, 256) and (blk.shortcut is not None) == (c1.cin == 64) and x.shape[-1] == c1.cin and x.is_contiguous())


def _reads_even_pixels_only(blk: BottleneckBlock) -> bool:
    """a stage's first block under STRIDE_IN_1X1: its input is read by two 1x1 stride-2 convolutions, i.e. at the pixels (2i, 2j) only"""
    sc, c1 = blk.shortcut, blk.conv1
    return sc is not None and all(c.k == 1 and c.stride == 2 and c.pad == 0 for c in (sc, c1))


def _tail_form(blk: BottleneckBlock, nxt: Optional[BottleneckBlock], x) -> bool:
    """The TAIL FORM of a bottleneck block: it is the last of its stage, the only reader of its output is a block that samples the even
    pixels, and the map is even-sized -- so three of every four output pixels are dead.  conv1 still runs on the whole map; conv2 runs as a
    3x3 stride-2 convolution and conv3 + FrozenBN + shortcut + ReLU on the quarter map; the next block's stride-2 1x1 convolutions become
    plain products on that compact tensor.  In the backward the dead pixels carried exact zeros: the same sums without them."""
    c1, c2, c3 = blk.conv1, blk.conv2, blk.conv3
    return (nxt is not None and _reads_even_pixels_only(nxt) and blk.shortcut is None and x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0
            and c1.k == 1 and c1.stride == 1 and c2.k == 3 and c2.stride == 1 and c2.pad == 1 and c3.k == 1 and c3.stride == 1
            and c1.cin % 8 == 0 and c2.cin % 8 == 0 and c3.cin % 8 == 0)


def blocks_forward(rt: Runtime, x, stages, save: bool, tail: bool = True):
    """The bottleneck blocks of ``stages`` (a list of block lists) on x (n, h, w, c) -> (output, saved).  saved: one record
    (blk, x, y1, y2, out, tail, compact_in) per trainable block when ``save``; tail: the block ran in its tail form (y2 and out hold the
    even pixels only); compact_in: x is such an output, and the block's stride-2 1x1 convolutions ran as plain products on it."""
    saved = []
    flat = [(blk, stage[i + 1] if i + 1 < len(stage) else (stages[si + 1][0] if si + 1 < len(stages) and stages[si + 1] else None), i + 1 == len(stage))
            for si, stage in enumerate(stages) for i, blk in enumerate(stage)]
    compact_in = False
    for blk, nxt, last in flat:
        if not compact_in and _res2_fusable(rt, x, blk, save):
            x = _res2_block_fused(rt, x, blk)
            continue
        as_tail = tail and last and _tail_form(blk, nxt, x)
        c1, csc = (_ConvAs(blk.conv1, 1), _ConvAs(blk.shortcut, 1)) if compact_in else (blk.conv1, blk.shortcut)
        sc = _conv_fwd(rt, x, csc) if blk.shortcut is not None else x
        y1 = _conv_fwd(rt, x, c1, act=ACT_RELU)
        if as_tail:
            n, h, w, _ = x.shape
            y2 = _conv_fwd(rt, y1, _ConvAs(blk.conv2, 2), act=ACT_RELU)
            out = _conv_fwd(rt, y2, blk.conv3, residual=sc, relu_after=True, res_rowmap=rt.rowmap(even_pixel_rows, n, h, w, x.device))
        else:
            y2 = _conv_fwd(rt, y1, blk.conv2, act=ACT_RELU)
            out = _conv_fwd(rt, y2, blk.conv3, residual=sc, relu_after=True)
        if save and _block_trainable(rt, blk):
            saved.append((blk, x, y1, y2, out, as_tail, compact_in))
        x, compact_in = out, as_tail
    return x, saved


def _stem_forward(bb: "GridFeatBackbone", x5):
    """frames -> stem convolution + FrozenBN + ReLU + 3x3/2 max-pool (n, h/4, w/4, 64).  Raw frames / uint8 / float input, each
    through the fused launch (bf16, even width: the 112 x 112 x 64 map never leaves the CU) or as packed image -> GEMM -> pool."""
    rt = bb.rt
    b, t, c, h, w = x5.shape
    n = b * t
    stem = bb.feature.backbone.stem.conv1
    oh, ow = _out_hw(h, w, 7, 2, 3)
    fused = rt.dtype == torch.bfloat16 and w % 2 == 0
    if isinstance(x5, RawFrames):
        # ImageResize + ImagePad + ImageNorm + BGR flip of the whole ragged batch in one launch, straight into the stem's packed image
        table, host_table = x5.packed_table()
        # (an indirect one -- the static input of a captured step -- names its bytes by a descriptor the kernel reads: the _src entry points)
        where = dict(host_table=host_table) if x5.source is None else dict(source=x5.source)
        if x5.pixfmt == "rgb":
            packed = ops.resize_pack_u8(x5.flat, table, n, h, rt.dtype, bb.pixel_mean, bb.pixel_std, hwc=x5.hwc, pad=3, extra_w=2, **where)
        else:                                           # the decoder's YUV 4:2:0 planes: the colour conversion rides in the same launch
            packed = ops.resize_pack_yuv420(x5.flat, table, n, h, rt.dtype, bb.pixel_mean, bb.pixel_std, layout=x5.pixfmt, matrix=x5.matrix,
                                            pad=3, extra_w=2, **where)
    else:
        x4 = x5.reshape(n, c, h, w)
        if not x4.is_contiguous():
            x4 = x4.contiguous()
        u8 = x4.dtype == torch.uint8
        if u8 and fused:
            # uint8 frames straight into the first convolution: ImageNorm, BGR flip and padding inside cb_stem_pool's tile loader
            return ops.stem_pool_u8(x4, bb.pixel_mean, bb.pixel_std, _stem_weight(rt, stem), *stem.scale_shift())
        packed = ops.stem_pack(x4, rt.dtype, 3, bb.pixel_mean, bb.pixel_std, extra_w=2) if u8 else ops.stem_pack(x4.float(), rt.dtype, 3, extra_w=2)
    scale, shift = stem.scale_shift()
    if fused:
        return ops.stem_pool(packed, _stem_weight(rt, stem), scale, shift, oh, ow)
    # the packed image is (n, hp, wp, 4): a window is 7 rows of 8 taps x 4 channels, every other pixel, no padding left to apply
    hp, wp = packed.shape[1], packed.shape[2]
    y = torch.empty(n, oh, ow, 64, dtype=rt.dtype, device=x5.device)
    ops.gemm(packed, _stem_weight(rt, stem), n * oh * ow, 64, 224, out=y.view(-1, 64), ldb=224,
             **conv_gather(rt, "a", n, hp, wp, 4, 7, 2, 0, x5.device, out_hw=(oh, ow), taps=(7, 1, 32)), scale=scale, shift=shift, act=ACT_RELU)
    return ops.maxpool_fwd(y, 3, 2, 1)


def cnn_forward(bb: "GridFeatBackbone", x5, save: bool):
    """(B,T,3,H,W) fp32 RGB mean-subtracted (or uint8 RGB), or the RawFrames standing for such a batch (native-resolution uint8
    frames: resized, padded and normalised here) -> grid (B,T,H',W',hidden) + saved activations."""
    rt = bb.rt
    b, t = x5.shape[:2]
    net = bb.feature.backbone
    x = _stem_forward(bb, x5)
    x, saved = blocks_forward(rt, x, [list(getattr(net, name)) for name, *_ in RESNET50_STAGES], save)
    gconv = bb.grid_encoder[0]
    gy = _conv_fwd(rt, x, gconv)
    grid = ops.maxpool_fwd(gy, 2, 2, 0, relu=True)
    return grid.view(b, t, *grid.shape[1:]), (saved, x, gy, grid) if save else None


def cnn_backward(bb: "GridFeatBackbone", saved_pack, dgrid: torch.Tensor):
    """the whole ResNet backward; rt.after_res5_backward (if set) is called at the point cnn_backward_steps yields, when this is the
    last pending ResNet backward of the step"""
    for _ in cnn_backward_steps(bb, saved_pack, dgrid):
        bb.rt.fire_if_last("cnn")


def cnn_backward_steps(bb: "GridFeatBackbone", saved_pack, dgrid: torch.Tensor):
    """Generator over the ResNet backward.  Yields ONCE, when every launch that writes a gradient of grid_encoder or res5 (the tail
    of the CNN range of the flat gradient buffer, and ~3/4 of its bytes) has been enqueued and earlier stages remain: a
    data-parallel caller starts that part of the exchange there (hook above, or between two captured graphs: bench.py).  Exhausting
    it without looking at the yield is the plain backward."""
    rt = bb.rt
    saved, res5, gy, grid = saved_pack
    gconv = bb.grid_encoder[0]
    dg = ops.maxpool2_bwd(gy, grid, dgrid.reshape(grid.shape).contiguous(), relu=True)
    _conv_wgrad(rt, dg, res5, gconv)
    if not saved:
        return
    res5_ids = {id(b) for b in bb.feature.backbone.res5}
    first_res5 = min((i for i, rec in enumerate(saved) if id(rec[0]) in res5_ids), default=None)
    # weight gradients of a stage's convolutions: described as the data-gradient chain passes them, launched together when the chain
    # leaves the stage (cb_gemm_group)
    stage_of = {id(b): name for name, *_ in RESNET50_STAGES for b in getattr(bb.feature.backbone, name)}
    pend = []

    def flush():
        ops.gemm_group(pend, dg)
        pend.clear()

    # (g3, sec): g3 = d(conv3 output of the block), sec = d(identity shortcut) or d(shortcut conv output)
    g3, sec = _conv_dgrad(rt, dg, gconv, res5.shape, fuse=_fuse_spec(saved[-1]))
    yield from blocks_backward(rt, saved, g3, sec, stage_of, flush, pend, first_res5)


def _fuse_spec(rec):
    """the ReLU x FrozenBN-scale backward of a saved block, done by the launch that produces d(output of that block)"""
    b, o = rec[0], rec[4]
    s3_, _ = b.conv3.scale_shift()
    ssc_ = b.shortcut.scale_shift()[0] if b.shortcut is not None else None
    return (o, s3_, ssc_)


def blocks_backward(rt: Runtime, saved, g3, sec, stage_of, flush, pend, first_res5=None, dx_out=None):
    """Generator over the backward of the saved blocks (blocks_forward's records), last to first, from (g3, sec) of the last one; yields
    where cnn_backward_steps documents.  ``dx_out`` (a list): d(input of the first saved block) is computed too and appended.
    A tail-form block works on the quarter map from the launches that produce its (g3, sec) down to its conv2: the 3x3 stride-2 data
    gradient (one launch, by parity classes) is where the chain returns to the whole map, and the block's conv1 data gradient adds the
    compact identity-shortcut gradient at the even pixels through a row map."""
    for idx in range(len(saved) - 1, -1, -1):
        blk, x, y1, y2, out, tail, compact_in = saved[idx]
        need_dx = idx > 0 or dx_out is not None
        s2, _ = blk.conv2.scale_shift()
        s1, _ = blk.conv1.scale_shift()
        dz, gsc = (sec, None) if blk.shortcut is None else (None, sec)
        c1, csc = (_ConvAs(blk.conv1, 1), _ConvAs(blk.shortcut, 1)) if compact_in else (blk.conv1, blk.shortcut)
        c2 = _ConvAs(blk.conv2, 2) if tail else blk.conv2
        _conv_wgrad(rt, g3, y2, blk.conv3, pend)
        if blk.shortcut is not None:
            _conv_wgrad(rt, gsc, x, csc, pend)
        g2 = _conv_dgrad(rt, g3, blk.conv3, y2.shape, scale=s2, mask=y2)       # -> d(conv2 out) * mask * scale2
        _conv_wgrad(rt, g2, y1, c2, pend)
        g1 = _conv_dgrad(rt, g2, c2, y1.shape, scale=s1, mask=y1)
        _conv_wgrad(rt, g1, x, c1, pend)
        if idx == 0 or stage_of.get(id(saved[idx - 1][0])) != stage_of.get(id(blk)):
            flush()                                     # the chain leaves this stage: its weight gradients in a few grouped launches
        if idx == first_res5 and idx > 0:
            yield "grid_encoder+res5"
        if need_dx:
            n, h, w, _ = x.shape
            if idx > 0:
                spec = _fuse_spec(saved[idx - 1])
            if blk.shortcut is None:
                rmap = dict(res_rowmap=rt.rowmap(even_pixel_index, n, h, w, x.device)) if tail else {}
                if idx > 0:
                    g3, sec = _conv_dgrad(rt, g1, c1, x.shape, residual=dz, fuse=spec, **rmap)
                else:
                    dx_out.append(_conv_dgrad(rt, g1, c1, x.shape, residual=dz, **rmap))
            else:
                dout = _conv_dgrad(rt, g1, c1, x.shape)
                if idx > 0:
                    g3, sec = _conv_dgrad(rt, gsc, csc, x.shape, out=dout, accumulate=True, fuse=spec)
                else:
                    dx_out.append(_conv_dgrad(rt, gsc, csc, x.shape, out=dout, accumulate=True))


class _CnnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, x5, bb):
        save = ctx.needs_input_grad[0] and bb.has_trainable()    # anchor: True iff autograd is recording
        grid, pack = cnn_forward(bb, x5, save)
        ctx.bb, ctx.pack = bb, pack
        if pack is not None:
            bb.rt.pending_cnn_nodes += 1
        return grid

    @staticmethod
    def backward(ctx, dgrid):
        if ctx.pack is not None:
            cnn_backward(ctx.bb, ctx.pack, dgrid.contiguous())
            ctx.pack = None
            ctx.bb.rt.node_done("cnn")
        return None, None, None


class GridFeatBackbone(nn.Module):
    """ResNet-50 grid-feature backbone + grid encoder (src/modeling/grid_feat.py:37-105)."""
    def __init__(self, detectron2_model_cfg=None, config=None, input_format="BGR", freeze_at=2):
        super().__init__()
        assert input_format == "BGR", "detectron 2 image input format should be BGR"
        config = as_config(config)
        self.detectron2_model_cfg = detectron2_model_cfg
        self.feature = _Detectron2Model()
        self.grid_encoder = nn.ModuleList([_GridConv(config.backbone_channel_in_size, config.hidden_size)])
        self.input_format = input_format
        self.config = config
        self.pixel_mean = (123.675, 116.28, 103.53)
        self.pixel_std = (1.0, 1.0, 1.0)
        self.rt: Optional[Runtime] = None
        # detectron2 FREEZE_AT=2: stem and res2 never receive gradients
        net = self.feature.backbone
        frozen = [net.stem] + ([net.res2] if freeze_at >= 2 else [])
        for mod in frozen:
            for p in mod.parameters():
                p.requires_grad = False

    @property
    def config_file(self):
        return f"clipbert_amd R-50 grid backbone (detectron2 cfg: {self.detectron2_model_cfg})"

    def has_trainable(self):
        return any(p.requires_grad for p in self.parameters())

    def forward(self, x):
        """x: (B, n_frm, 3, H, W) RGB float (mean-subtracted) or uint8, or a data.RawFrames of that shape -> (B, n_frm, H', W', hidden)."""
        return _CnnFn.apply(self.rt.anchor, x, self)


def cnn_early_split(model) -> Optional[int]:
    """Element offset in the flat gradient buffer where res5's parameters start (they are the tail of the CNN range: same module
    order as the reference's parameter groups); None when res5 is frozen or not contiguous at the end.  GradSync.set_cnn_split."""
    bank = model.rt.bank
    ps = [p for p in model.cnn.feature.backbone.res5.parameters() if bank.is_trainable(p)]
    if not ps:
        return None
    start = min(bank.offset[id(p)] for p in ps)
    g6 = bank.group_range[6]
    others = [bank.offset[id(p)] for n, p in model.cnn.feature.backbone.named_parameters()
              if bank.is_trainable(p) and not n.startswith("res5.")]
    if not (g6[0] <= start < g6[1]) or any(o >= start for o in others):
        return None
    return start
