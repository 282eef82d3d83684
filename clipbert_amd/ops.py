"""Tensor-level wrappers over the C ABI (raw device pointers + current HIP stream).

These are plumbing only: argument marshalling, output allocation with torch (device memory), and
error propagation.  All arithmetic happens in libclipbert_hip.so.
"""
import ctypes as C
import os
from typing import Optional

import torch

from . import _lib
from ._lib import (ACT_GELU, ACT_GELU_SAVE_GRAD, ACT_NONE, ACT_RELU, ACT_SAVED_GRAD, ACT_TANH, CB_BF16, CB_F32, KROW, KROW_GATHER,  # noqa: F401
                   KROW_TAPS, ROWK, ROWK_GATHER, GemmDesc)

# Set only by the CPU test-suite when it swaps in the host emulator build of the same sources.
_ALLOW_HOST_POINTERS = False


def dtype_code(t: torch.dtype) -> int:
    if t == torch.bfloat16:
        return CB_BF16
    if t == torch.float32:
        return CB_F32
    raise TypeError(f"unsupported dtype {t}")


def _ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda and not _ALLOW_HOST_POINTERS:
        raise RuntimeError("clipbert_amd ops need CUDA(HIP) tensors: there is no CPU path")
    return t.data_ptr()


def _extent_bytes(t: torch.Tensor) -> int:
    """bytes from data_ptr() to the end of the tensor's storage (upper bound of any strided view)"""
    return t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()


def _stream(t: torch.Tensor):
    if t.is_cuda:
        return torch.cuda.current_stream(t.device).cuda_stream
    return None


def _chk(rc, what):
    _lib.check(rc, what)


def gemm_desc(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, *, out: torch.Tensor, a_mode=ROWK,
              b_mode=ROWK, lda=None, ldb=None, ldc=None, a_tab=None, b_tab=None, R=1, S=1, Cin=0, H=0, W=0,
              sH=0, sW=0, flip_taps=False, c_rowmap=None, accumulate=False, split_k=1, act=ACT_NONE,
              scale=None, shift=None, residual=None, ldr=None, relu_after=False, mask=None, ldm=None,
              out2=None, ldc2=None, alpha=1.0, dropout_p=0.0, dropout_seed=0, seed_ptr=None, tile=0, gelu_grad_pre=None, a_rowsum=None, batch=1, batch_strides=None,
              relu_bwd=False, post_scale=None, post_scale2=None, xcd_order=0, zero_fill_pitch=0, splitk_ws=None, schedule=0, sq_slots=None,
              res_rowmap=None, dgrad_s2=False) -> GemmDesc:
    """The cb_gemm_desc of C[M,N] (op)= epilogue(sum_k A(m,k) B(n,k)); see include/clipbert_hip.h.  ``splitk_ws``: fp32 scratch for
    the K split of the 8-wave tiles (default: the per-device workspace of ``splitk_workspace``).  The descriptor borrows the
    tensors' memory: the caller keeps them alive until the launch that consumes it has been enqueued (``_refs`` holds them)."""
    d = GemmDesc()
    d.dtype = dtype_code(a.dtype)
    assert b.dtype == a.dtype
    d.M, d.N, d.K = M, N, K
    d.a_mode, d.b_mode = a_mode, b_mode
    d.A, d.B = _ptr(a), _ptr(b)
    d.lda = lda if lda is not None else a.stride(0)
    d.ldb = ldb if ldb is not None else b.stride(0)
    d.a_tab, d.b_tab = _ptr(a_tab), _ptr(b_tab)
    d.R, d.S, d.Cin, d.H, d.W, d.sH, d.sW = R, S, Cin, H, W, sH, sW
    d.flip_taps = int(flip_taps)
    d.C = _ptr(out)
    d.ldc = ldc if ldc is not None else out.stride(0)
    d.c_rowmap = _ptr(c_rowmap)
    d.zero_fill_pitch = zero_fill_pitch
    d.c_f32 = int(out.dtype == torch.float32)
    d.accumulate = int(accumulate)            # False / True, or 2 = first writer (C holds nothing; stored; K split only through slabs)
    d.split_k = split_k
    d.act = act
    d.scale, d.shift = _ptr(scale), _ptr(shift)
    d.residual = _ptr(residual)
    d.ldr = (ldr if ldr is not None else residual.stride(0)) if residual is not None else 0
    if res_rowmap is not None:                # the residual through its own int32 row map (entry -1: none for that row)
        assert residual is not None and res_rowmap.dtype == torch.int32 and res_rowmap.numel() == M
        d.res_rowmap, d.res_rows = _ptr(res_rowmap), residual.shape[0]
    d.dgrad_s2 = int(dgrad_s2)                # 3x3 stride-2 data gradient by parity classes (cb_gemm_desc.dgrad_s2)
    d.relu_after = int(relu_after)
    d.mask = _ptr(mask)
    d.ldm = (ldm if ldm is not None else mask.stride(0)) if mask is not None else 0
    d.C2 = _ptr(out2)
    d.ldc2 = (ldc2 if ldc2 is not None else out2.stride(0)) if out2 is not None else 0
    d.alpha = alpha
    d.dropout_p = dropout_p
    d.dropout_seed = dropout_seed
    d.dropout_seed_ptr = _ptr(seed_ptr)
    if _KEY_LOG is not None:                 # tools/tune_instep.py: the problem shapes of a step
        _KEY_LOG.append((a_mode, b_mode, M, N, K, batch, R * S, split_k))
    if tile == 0 and _LAUNCH_OVERRIDE:       # tools/tune_instep.py: a launch configuration under test for this problem shape
        ov = _LAUNCH_OVERRIDE.get((a_mode, b_mode, M, N, K, batch, R * S, split_k))
        if ov is not None:
            tile, xcd_order, schedule = ov[0], ov[1], ov[3]
            d.split_k = ov[2] if ov[2] > 0 else split_k
    d.tile = tile
    d.schedule = schedule
    d.xcd_order = xcd_order
    d.a_bytes = _extent_bytes(a)
    d.b_bytes = _extent_bytes(b)
    if gelu_grad_pre is not None:
        d.gelu_grad_pre, d.ld_gelu = _ptr(gelu_grad_pre), gelu_grad_pre.stride(0)
    if a_rowsum is not None:
        assert a_rowsum.dtype == torch.float32
        d.a_rowsum = _ptr(a_rowsum)
    if relu_bwd:
        d.relu_bwd = 1
        d.post_scale, d.post_scale2 = _ptr(post_scale), _ptr(post_scale2)
    if batch > 1:
        d.batch = batch
        d.batch_stride_a, d.batch_stride_b, d.batch_stride_c, d.batch_stride_rowsum = batch_strides
    if splitk_ws is None and d.dtype == CB_BF16 and not _SPLITK_OFF:
        splitk_ws = splitk_workspace(a.device)
    if splitk_ws is not None:
        d.splitk_ws, d.splitk_ws_bytes = _ptr(splitk_ws), splitk_ws.numel() * splitk_ws.element_size()
    if sq_slots is not None:                  # fp32 slots for the tiles' shares of sum(C^2) (cb_gemm_desc.sq_slots)
        assert sq_slots.dtype == torch.float32 and sq_slots.is_contiguous()
        d.sq_slots, d.sq_slots_n = _ptr(sq_slots), sq_slots.numel()
    d._refs = (a, b, out, a_tab, b_tab, c_rowmap, scale, shift, residual, mask, out2, seed_ptr, gelu_grad_pre, a_rowsum, post_scale,
               post_scale2, splitk_ws, sq_slots, res_rowmap)
    return d


def gemm(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, *, out: torch.Tensor, **kw):
    """C[M,N] (op)= epilogue(sum_k A(m,k) B(n,k)): one cb_gemm launch on a's current stream (arguments: gemm_desc)."""
    d = gemm_desc(a, b, M, N, K, out=out, **kw)
    _chk(_lib.get().cb_gemm(C.byref(d), _stream(a)), "cb_gemm")
    return out


def gemm_plan(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, *, out: torch.Tensor, use_table: bool = True, **kw):
    """cb_gemm_plan: (tile, split_k, schedule, xcd_order) cb_gemm would launch this call with; launches nothing."""
    d = gemm_desc(a, b, M, N, K, out=out, **kw)
    plan = (C.c_int32 * 4)()
    _chk(_lib.get().cb_gemm_plan(C.byref(d), 1 if use_table else 0, plan), "cb_gemm_plan")
    return tuple(plan)


def gemm_group(descs, like: torch.Tensor):
    """cb_gemm_group: the INDEPENDENT problems ``descs`` (gemm_desc results; no output overlaps another problem's output or
    operands) in as few launches as the library manages, on ``like``'s current stream."""
    n = len(descs)
    if n == 0:
        return
    arr = (GemmDesc * n)()
    for i, d in enumerate(descs):
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(GemmDesc))
    _chk(_lib.get().cb_gemm_group(C.cast(arr, C.c_void_p), n, _stream(like)), "cb_gemm_group")


_KEY_LOG = None                        # a list while tools/tune_instep.py records the keys of a step's problems
_LAUNCH_OVERRIDE = {}                  # (a_mode, b_mode, M, N, K, batch, taps, split_k) -> (tile, xcd_order, split_k, schedule); tuning only
_TILE_ID = {"128x128": 1, "64x64": 2, "128x64": 3, "128x128o2": 4, "8w256x256": 5, "8w128x256": 6, "8w256x128": 7}


def parse_launch_config(name: str):
    """'8w256x256/xcd/s1/m0' -> (tile, xcd_order, split_k, schedule): the configuration names of tools/tune_gemm.py"""
    parts = name.split("/")
    tile = _TILE_ID[parts[0]]
    xcd = 1 if parts[1] == "xcd" else 2
    split = ([int(x[1:]) for x in parts[2:] if x[0] == "s"] or [0])[0]
    sched = ([int(x[1:]) + 1 for x in parts[2:] if x[0] == "m"] or [0])[0]
    return (tile, xcd, split or (1 if tile >= 5 else 0), sched)


# diagnostics (A/B calls): CB_LAUNCH_OVERRIDE="a_mode,b_mode,M,N,K,batch,taps,split_k=config;..." pins launch configurations of problem shapes
for _item in filter(None, os.environ.get("CB_LAUNCH_OVERRIDE", "").split(";")):
    _k, _, _c = _item.partition("=")
    _LAUNCH_OVERRIDE[tuple(int(x) for x in _k.split(","))] = parse_launch_config(_c)
_SPLITK_WS = {}
_SPLITK_OFF = False                    # True: descriptors get no K-split scratch (split launches add through fp32 atomics; tests of that path)
SPLITK_WS_BYTES = 128 << 20


def splitk_workspace(device) -> torch.Tensor:
    """One fp32 scratch buffer per device for the K-split partial products of cb_gemm's 8-wave tiles.  Launches that follow one
    another on a stream (or on streams ordered by events, as a hipGraph capture after an eager warm-up) share it; launches on a
    concurrent stream need a scratch of their own (new_splitk_workspace).  Allocated on first use / by ClipBert.prepare(), never inside a
    capture."""
    dev = torch.device(device)
    key = str(dev)
    ws = _SPLITK_WS.get(key)
    if ws is None:
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return None
        ws = new_splitk_workspace(device)
        _SPLITK_WS[key] = ws
    return ws


def new_splitk_workspace(device, nbytes: int = SPLITK_WS_BYTES) -> torch.Tensor:
    """A K-split scratch as include/clipbert_hip.h lays it out: partial products, then CB_SPLITK_WS_COUNTER_BYTES of arrival counters
    that start at zero (every launch leaves them zero).  One per stream whose launches may overlap another stream's."""
    assert nbytes % 16 == 0 and nbytes > _lib.SPLITK_WS_COUNTER_BYTES
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    ws[-(_lib.SPLITK_WS_COUNTER_BYTES // 4):].zero_()
    return ws


def build_pixel_table(n: int, oh: int, ow: int, stride: int, pad: int, sN: int, sH: int, sW: int,
                      device) -> torch.Tensor:
    """int64 tensor viewed as cb_pixel {int32 off; int16 ih0; int16 iw0} entries."""
    tab = torch.empty(n * oh * ow, dtype=torch.int64, device=device)
    _chk(_lib.get().cb_build_pixel_table(_ptr(tab), n, oh, ow, stride, pad, sN, sH, sW, _stream(tab)),
         "cb_build_pixel_table")
    return tab


def _f3(vals):
    return (C.c_float * 3)(*[float(v) for v in vals])


def stem_pack(src: torch.Tensor, dtype: torch.dtype, pad: int = 3, mean=None, std=None, extra_w: int = 0) -> torch.Tensor:
    """(N,3,H,W) fp32 (already normalised) or uint8 (+mean/std) -> (N, H+2*pad, W+2*pad+extra_w, 4) zero-padded BGR0."""
    n, c, h, w = src.shape
    assert c == 3 and src.is_contiguous()
    hp, wp = h + 2 * pad, w + 2 * pad + extra_w
    dst = torch.empty(n, hp, wp, 4, dtype=dtype, device=src.device)
    u8 = src.dtype == torch.uint8
    assert u8 or src.dtype == torch.float32
    m3 = _f3(mean) if u8 else None
    s3 = _f3(std) if u8 else None
    _chk(_lib.get().cb_stem_pack(dtype_code(dtype), _ptr(src), int(u8), m3, s3, _ptr(dst), n, h, w, hp, wp, pad,
                                 _stream(src)), "cb_stem_pack")
    return dst


def _resize_pack_args(flat_u8, table, n, host_table, source):
    """what the two ingest wrappers ask of their tensors -> the device the image is written on"""
    assert table.dtype == torch.int64 and tuple(table.shape) == (n, 5) and table.is_contiguous()
    if source is not None:
        assert flat_u8 is None and host_table is None, "source=: the bytes are named by the descriptor, and the launch validates no host table (resize_table_check)"
        assert source.dtype in (torch.uint8, torch.int64) and source.numel() * source.element_size() == 16 and source.is_contiguous()
        assert source.device == table.device and source.data_ptr() % 16 == 0
        return table.device
    assert flat_u8.dtype == torch.uint8 and flat_u8.dim() == 1 and flat_u8.is_contiguous() and table.device == flat_u8.device
    if host_table is not None:
        assert host_table.dtype == torch.int64 and tuple(host_table.shape) == (n, 5) and host_table.is_contiguous() and not host_table.is_cuda
    return flat_u8.device


def resize_pack_u8(flat_u8: Optional[torch.Tensor], table: torch.Tensor, n: int, size: int, dtype: torch.dtype, mean, std, hwc: bool = True,
                   pad: int = 3, extra_w: int = 0, host_table: Optional[torch.Tensor] = None, source: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cb_resize_pack_u8: ``n`` native-resolution uint8 RGB frames lying back to back in ``flat_u8`` -> the reference's bilinear
    resize (longer side -> ``size``) + zero pad to size x size + ImageNorm, as stem_pack's (n, size+2*pad, size+2*pad+extra_w, 4)
    BGR0 image.  ``table``: int64 (n, 5) rows [byte_offset, h, w, new_h, new_w] on flat_u8's device (clipbert_amd.data.RawFrames
    builds it); ``host_table``: a CPU copy whose rows the library validates before the launch.  One launch, no host sync.

    ``source`` (with ``flat_u8`` None): cb_resize_pack_u8_src -- a cb_frame_source descriptor on the table's device, uint8 (16,) or
    int64 (2,) [base address, byte count], read by the kernel at run time: the launch depends on no address or size of the batch, so
    a captured one serves every batch.  Bit-equal to the direct call on the same bytes; no host table is validated."""
    dev = _resize_pack_args(flat_u8, table, n, host_table, source)
    hp, wp = size + 2 * pad, size + 2 * pad + extra_w
    dst = torch.empty(n, hp, wp, 4, dtype=dtype, device=dev)
    if source is not None:
        _chk(_lib.get().cb_resize_pack_u8_src(dtype_code(dtype), _ptr(source), _ptr(table), n, int(hwc), _f3(mean), _f3(std), _ptr(dst), size, hp,
                                              wp, pad, _stream(table)), "cb_resize_pack_u8_src")
        return dst
    _chk(_lib.get().cb_resize_pack_u8(dtype_code(dtype), _ptr(flat_u8), flat_u8.numel(), _ptr(table),
                                      host_table.data_ptr() if host_table is not None else None, n, int(hwc), _f3(mean), _f3(std),
                                      _ptr(dst), size, hp, wp, pad, _stream(flat_u8)), "cb_resize_pack_u8")
    return dst


def resize_pack_yuv420(flat_u8: Optional[torch.Tensor], table: torch.Tensor, n: int, size: int, dtype: torch.dtype, mean, std, layout: str = "i420",
                       matrix: str = "bt601", pad: int = 3, extra_w: int = 0, host_table: Optional[torch.Tensor] = None,
                       source: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cb_resize_pack_yuv420: resize_pack_u8 for ``n`` YUV 4:2:0 frames lying back to back in ``flat_u8`` as their tightly packed
    planes -- ``layout`` "i420" (Y, U, V) or "nv12" (Y, interleaved UV), h * w + 2 * ceil(h / 2) * ceil(w / 2) bytes each -- converted
    with ``matrix`` ("bt601", "bt601-full", "bt709", "bt709-full"; nearest chroma) tap by tap.  Bit-equal to resize_pack_u8(hwc=False)
    on the converted uint8 RGB frames.  ``table`` / ``host_table`` / ``source`` (cb_resize_pack_yuv420_src) as there.  One launch, no
    host sync."""
    dev = _resize_pack_args(flat_u8, table, n, host_table, source)
    hp, wp = size + 2 * pad, size + 2 * pad + extra_w
    dst = torch.empty(n, hp, wp, 4, dtype=dtype, device=dev)
    if source is not None:
        _chk(_lib.get().cb_resize_pack_yuv420_src(dtype_code(dtype), _ptr(source), _ptr(table), n, _lib.YUV_LAYOUTS[layout], _lib.YUV_MATRICES[matrix],
                                                  _f3(mean), _f3(std), _ptr(dst), size, hp, wp, pad, _stream(table)), "cb_resize_pack_yuv420_src")
        return dst
    _chk(_lib.get().cb_resize_pack_yuv420(dtype_code(dtype), _ptr(flat_u8), flat_u8.numel(), _ptr(table),
                                          host_table.data_ptr() if host_table is not None else None, n, _lib.YUV_LAYOUTS[layout],
                                          _lib.YUV_MATRICES[matrix], _f3(mean), _f3(std), _ptr(dst), size, hp, wp, pad, _stream(flat_u8)),
         "cb_resize_pack_yuv420")
    return dst


def resize_table_check(host_table: torch.Tensor, n: int, flat_bytes: int, size: int, pixfmt: str = "rgb") -> None:
    """cb_resize_table_check: the row rules of the two direct entry points on a HOST table against a buffer of ``flat_bytes`` bytes, no
    launch -- what a replayed step runs on a batch before it stages it.  Raises the RuntimeError the direct launch would have raised
    (the same text, the direct entry point's name included)."""
    assert host_table.dtype == torch.int64 and tuple(host_table.shape) == (n, 5) and host_table.is_contiguous() and not host_table.is_cuda
    _chk(_lib.get().cb_resize_table_check(host_table.data_ptr(), n, int(flat_bytes), size, _lib.PIXFMTS[pixfmt]),
         "cb_resize_pack_u8" if pixfmt == "rgb" else "cb_resize_pack_yuv420")


def image_norm(frames_u8: torch.Tensor, mean, std) -> torch.Tensor:
    """ImageNorm (a1): uint8 (..., 3, H, W) -> fp32."""
    assert frames_u8.dtype == torch.uint8 and frames_u8.is_contiguous() and frames_u8.shape[-3] == 3
    out = torch.empty(frames_u8.shape, dtype=torch.float32, device=frames_u8.device)
    hw = frames_u8.shape[-1] * frames_u8.shape[-2]
    n = frames_u8.numel() // (3 * hw)
    _chk(_lib.get().cb_image_norm(_ptr(frames_u8), _ptr(out), _f3(mean), _f3(std), n, hw, _stream(out)),
         "cb_image_norm")
    return out


def maxpool_fwd(x: torch.Tensor, k: int, stride: int, pad: int, relu: bool = False) -> torch.Tensor:
    """x (N,H,W,C) NHWC."""
    n, h, w, c = x.shape
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    y = torch.empty(n, oh, ow, c, dtype=x.dtype, device=x.device)
    _chk(_lib.get().cb_maxpool_fwd(dtype_code(x.dtype), _ptr(x), _ptr(y), n, h, w, c, oh, ow, k, stride, pad,
                                   int(relu), _stream(x)), "cb_maxpool_fwd")
    return y


def stem_pool(packed, weight, scale, shift, oh: int, ow: int) -> torch.Tensor:
    """cb_stem_pool: stem convolution + FrozenBN + ReLU + 3x3/2 max-pool of the packed (N, Hp, Wp, 4) bf16 image in one launch ->
    (N, PH, PW, 64)."""
    n, hp, wp, _ = packed.shape
    assert packed.dtype == torch.bfloat16 and packed.is_contiguous() and weight.dtype == torch.bfloat16
    ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    out = torch.empty(n, ph, pw, 64, dtype=packed.dtype, device=packed.device)
    _chk(_lib.get().cb_stem_pool(_ptr(packed), _ptr(weight), _ptr(scale), _ptr(shift), _ptr(out), n, hp, wp, oh, ow, ph, pw, _stream(packed)),
         "cb_stem_pool")
    return out


def stem_pool_u8(frames: torch.Tensor, mean, std, weight, scale, shift) -> torch.Tensor:
    """cb_stem_pool_u8: (N, 3, H, W) uint8 RGB frames -> (N, PH, PW, 64) bf16: ImageNorm + BGR flip + zero padding + stem convolution + FrozenBN
    + ReLU + 3x3/2 max-pool in one launch (cb_stem_pack folded into cb_stem_pool; bit-identical to the two launches)."""
    n, c, h, w = frames.shape
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and c == 3 and weight.dtype == torch.bfloat16
    oh, ow = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
    out = torch.empty(n, ph, pw, 64, dtype=torch.bfloat16, device=frames.device)
    _chk(_lib.get().cb_stem_pool_u8(_ptr(frames), _f3(mean), _f3(std), _ptr(weight), _ptr(scale), _ptr(shift), _ptr(out), n, h, w, oh, ow, ph, pw,
                                    _stream(frames)), "cb_stem_pool_u8")
    return out


def res2_block(x, w1, w2, w3, ss1, ss2, ss3, wsc=None, sssc=None) -> torch.Tensor:
    """cb_res2_block: one res2 bottleneck block (64 mid channels, stride 1, FrozenBN, forward only) in one launch.  x (N, H, W, cin) bf16
    NHWC; w*: the convolutions' KRSC weight images; ss*: their (scale, shift) fp32 vectors; wsc / sssc: the projection shortcut of the
    stage-entry block (cin = 64), None for an identity shortcut (cin = 256)."""
    n, h, w, cin = x.shape
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    out = torch.empty(n, h, w, 256, dtype=x.dtype, device=x.device)
    d = _lib.Res2Desc()
    d.x, d.out = _ptr(x), _ptr(out)
    d.w1, d.w2, d.w3, d.wsc = _ptr(w1), _ptr(w2), _ptr(w3), _ptr(wsc)
    d.scale1, d.shift1, d.scale2, d.shift2, d.scale3, d.shift3 = (_ptr(t) for t in (*ss1, *ss2, *ss3))
    d.scale_sc, d.shift_sc = (_ptr(sssc[0]), _ptr(sssc[1])) if sssc is not None else (None, None)
    d.N, d.H, d.W, d.cin = n, h, w, cin
    d._refs = (x, out, w1, w2, w3, wsc, ss1, ss2, ss3, sssc)
    _chk(_lib.get().cb_res2_block(C.byref(d), _stream(x)), "cb_res2_block")
    return out


def maxpool2_bwd(x, y, dy, relu: bool = False) -> torch.Tensor:
    n, h, w, c = x.shape
    oh, ow = y.shape[1], y.shape[2]
    dx = torch.empty_like(x)
    _chk(_lib.get().cb_maxpool2_bwd(dtype_code(x.dtype), _ptr(x), _ptr(y), _ptr(dy), _ptr(dx), n, h, w, c, oh, ow,
                                    int(relu), _stream(x)), "cb_maxpool2_bwd")
    return dx


def relu_scale_bwd(dy, y, scale=None, want_dz=False, scale2=None):
    """returns (g = dy*(y>0)*scale | None, dz = dy*(y>0) | None, g2 = dz*scale2 | None)."""
    c = y.shape[-1]
    rows = y.numel() // c
    g = torch.empty_like(y) if scale is not None else None
    dz = torch.empty_like(y) if want_dz else None
    g2 = torch.empty_like(y) if scale2 is not None else None
    _chk(_lib.get().cb_relu_scale_bwd(dtype_code(y.dtype), _ptr(dy), _ptr(y), _ptr(scale), _ptr(g), _ptr(dz),
                                      _ptr(scale2), _ptr(g2), rows, c, _stream(y)), "cb_relu_scale_bwd")
    return g, dz, g2


def layernorm_fwd(x, gamma, beta, eps, save_stats=False, out=None):
    d = x.shape[-1]
    rows = x.numel() // d
    y = out if out is not None else torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device) if save_stats else None
    _chk(_lib.get().cb_layernorm_fwd(dtype_code(x.dtype), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean),
                                     _ptr(rstd), rows, d, eps, 0, 0, 0, _stream(x)), "cb_layernorm_fwd")
    return y, mean, rstd


def layernorm_bwd(dy, x, gamma, mean, rstd, dgamma, dbeta, dropout_p=0.0, dropout_seed=0, seed_ptr=None,
                  dx=None, rows=None, seg=(0, 0, 0), dx2=None):
    """returns (dx, dx_dropped|None); dgamma/dbeta (fp32) are accumulated in place.
    seg = (seg_len, seg_stride, seg_off) addresses a strided subset of rows (see the header)."""
    d = x.shape[-1]
    rows = x.numel() // d if rows is None else rows
    dx = torch.empty_like(x) if dx is None else dx
    dx2 = (dx2 if dx2 is not None else torch.empty_like(x)) if dropout_p > 0 else None
    _chk(_lib.get().cb_layernorm_bwd(dtype_code(x.dtype), _ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd),
                                     _ptr(dx), _ptr(dgamma), _ptr(dbeta), rows, d, _ptr(dx2), dropout_p,
                                     dropout_seed, _ptr(seed_ptr), seg[0], seg[1], seg[2], _stream(x)),
         "cb_layernorm_bwd")
    return dx, dx2


def ln_part_blocks(rows: int) -> int:
    """blocks cb_layernorm_bwd_part is launched with for `rows` rows (one row per wave, 12 waves per block, <= 256 blocks)"""
    return max(1, min(256, (rows + 11) // 12))


def layernorm_bwd_part(dy, x, gamma, mean, rstd, part, dropout_p=0.0, dropout_seed=0, seed_ptr=None, dx=None, dx2=None):
    """LayerNorm backward whose parameter-gradient partial sums go to part (nblocks, 2, D) fp32 (plain stores; ln_partials_reduce
    adds them to the gradients later).  returns (dx, dx_dropped|None)"""
    d = x.shape[-1]
    rows = x.numel() // d
    nblocks = part.shape[0]
    assert part.dtype == torch.float32 and part.is_contiguous() and part.shape[1:] == (2, d)
    dx = torch.empty_like(x) if dx is None else dx
    dx2 = (dx2 if dx2 is not None else torch.empty_like(x)) if dropout_p > 0 else None
    _chk(_lib.get().cb_layernorm_bwd_part(dtype_code(x.dtype), _ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx),
                                          _ptr(part), nblocks, rows, d, _ptr(dx2), dropout_p, dropout_seed, _ptr(seed_ptr),
                                          0, 0, 0, _stream(x)), "cb_layernorm_bwd_part")
    return dx, dx2


def ln_partials_reduce(part, grad, off_gamma, off_beta):
    """grad[off_gamma[j] + c] += sum_b part[j, b, 0, c]; grad[off_beta[j] + c] += sum_b part[j, b, 1, c]  (fixed order)"""
    njobs, nblocks, two, d = part.shape
    assert two == 2 and part.is_contiguous() and off_gamma.dtype == torch.int64 and off_gamma.numel() == njobs == off_beta.numel()
    _chk(_lib.get().cb_ln_partials_reduce(_ptr(part), _ptr(grad), _ptr(off_gamma), _ptr(off_beta), njobs, nblocks, d, _stream(part)),
         "cb_ln_partials_reduce")


def text_embed_fwd(ids, word, pos, type0, gamma, beta, out, pre, mean, rstd, lt, l_total, eps, attn_mask=None, key_mask=None,
                   repeat=1):
    """``repeat`` = n: the (P, Lt) ids / attn_mask are the text batch of ONE clip; n*P output rows are produced (row b reads row
    b % P).  ``key_mask`` (B, L_total) fp32 receives the text columns of the attention key mask."""
    b = ids.shape[0] * repeat
    d = word.shape[-1]
    _chk(_lib.get().cb_text_embed_fwd(dtype_code(word.dtype), _ptr(ids), _ptr(word), _ptr(pos), _ptr(type0),
                                      _ptr(gamma), _ptr(beta), _ptr(out), _ptr(pre), _ptr(mean), _ptr(rstd), b, lt,
                                      l_total, d, eps, _ptr(attn_mask), _ptr(key_mask), ids.shape[0] if repeat > 1 else 0,
                                      _stream(out)), "cb_text_embed_fwd")


def visual_embed_fwd(grid, src_row, sel, row_emb, col_emb, type0, gamma, beta, out, pre, mean, rstd, b, lv, lt,
                     l_total, eps, key_mask=None):
    _, t, hg, wg, d = grid.shape
    _chk(_lib.get().cb_visual_embed_fwd(dtype_code(grid.dtype), _ptr(grid), _ptr(src_row), _ptr(sel), _ptr(row_emb),
                                        _ptr(col_emb), _ptr(type0), _ptr(gamma), _ptr(beta), _ptr(out), _ptr(pre),
                                        _ptr(mean), _ptr(rstd), b, t, hg, wg, lv, lt, l_total, d, eps, _ptr(key_mask),
                                        _stream(out)), "cb_visual_embed_fwd")


def text_embed_bwd(dpre, ids, dword, dpos, dtype0, lt, l_total, pad_id, repeat=1):
    b = ids.shape[0] * repeat
    d = dword.shape[-1]
    _chk(_lib.get().cb_text_embed_bwd(dtype_code(dpre.dtype), _ptr(dpre), _ptr(ids), _ptr(dword), _ptr(dpos),
                                      _ptr(dtype0), b, lt, l_total, d, pad_id, ids.shape[0] if repeat > 1 else 0, _stream(dpre)),
         "cb_text_embed_bwd")


def mean_fwd(x: torch.Tensor) -> torch.Tensor:
    """scalar mean of a contiguous fp32 vector (the runners' loss.mean())"""
    out = torch.empty((), dtype=torch.float32, device=x.device)
    _chk(_lib.get().cb_mean_fwd(_ptr(x), x.numel(), _ptr(out), _stream(x)), "cb_mean_fwd")
    return out


def mean_bwd(dmean: torch.Tensor, n: int, like: torch.Tensor) -> torch.Tensor:
    dx = torch.empty(n, dtype=torch.float32, device=like.device)
    _chk(_lib.get().cb_mean_bwd(_ptr(dmean), n, _ptr(dx), _stream(like)), "cb_mean_bwd")
    return dx


def counter_add(counter: torch.Tensor, inc: int = 1):
    """*counter += inc on a device int64 word (the dropout seed word: advanced inside a captured step)"""
    assert counter.dtype == torch.int64 and counter.numel() == 1
    _chk(_lib.get().cb_counter_add(_ptr(counter), inc, _stream(counter)), "cb_counter_add")


def zero_(t: torch.Tensor) -> torch.Tensor:
    """t[...] = 0 for a contiguous tensor (or contiguous slice of one): cb_zero on t's stream"""
    assert t.is_contiguous()
    if t.numel():
        _chk(_lib.get().cb_zero(_ptr(t), t.numel() * t.element_size(), _stream(t)), "cb_zero")
    return t


def zero_many(tensors) -> None:
    """every (contiguous) tensor of the list = 0, four per launch (cb_zero_ranges) on the first one's stream"""
    ts = [t for t in tensors if t is not None and t.numel()]
    for i in range(0, len(ts), 4):
        chunk = ts[i:i + 4]
        if len(chunk) == 1:
            zero_(chunk[0])
            continue
        assert all(t.is_contiguous() for t in chunk)
        ptrs = (C.c_void_p * len(chunk))(*[_ptr(t) for t in chunk])
        nbytes = (C.c_int64 * len(chunk))(*[t.numel() * t.element_size() for t in chunk])
        _chk(_lib.get().cb_zero_ranges(ptrs, nbytes, len(chunk), _stream(chunk[0])), "cb_zero_ranges")


def copy_ranges(pairs) -> None:
    """dst[...] = src[...] for every (dst, src) pair of contiguous tensors with the same number of bytes, eight pairs per launch
    (cb_copy_ranges) on the first destination's stream: a collated batch into the static buffers of a captured step"""
    ps = [(d, s) for d, s in pairs if d.numel()]
    for d, s in ps:
        assert d.is_contiguous() and s.is_contiguous() and d.numel() * d.element_size() == s.numel() * s.element_size(), (d.shape, s.shape)
        assert d.device == s.device, (d.device, s.device)
    for i in range(0, len(ps), 8):
        chunk = ps[i:i + 8]
        dsts = (C.c_void_p * len(chunk))(*[_ptr(d) for d, _ in chunk])
        srcs = (C.c_void_p * len(chunk))(*[_ptr(s) for _, s in chunk])
        nbytes = (C.c_int64 * len(chunk))(*[d.numel() * d.element_size() for d, _ in chunk])
        _chk(_lib.get().cb_copy_ranges(dsts, srcs, nbytes, len(chunk), _stream(chunk[0][0])), "cb_copy_ranges")


def zeros(shape, dtype, device) -> torch.Tensor:
    return zero_(torch.empty(shape, dtype=dtype, device=device))


def visual_embed_bwd(dpre, src_row, sel, dgrid, drow, dcol, dtype0, b, lv, lt, l_total):
    _, t, hg, wg, d = dgrid.shape
    _chk(_lib.get().cb_visual_embed_bwd(dtype_code(dpre.dtype), _ptr(dpre), _ptr(src_row), _ptr(sel), _ptr(dgrid),
                                        _ptr(drow), _ptr(dcol), _ptr(dtype0), b, t, hg, wg, lv, lt, l_total, d,
                                        _stream(dpre)), "cb_visual_embed_bwd")


def attention_fwd(qkv, key_mask, b, l, h, save_lse=False, dropout_p=0.0, dropout_seed=0, seed_ptr=None, out=None):
    ctx = out if out is not None else torch.empty(b * l, h * 64, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(b * h * l, dtype=torch.float32, device=qkv.device) if save_lse else None
    _chk(_lib.get().cb_attention_fwd(dtype_code(qkv.dtype), _ptr(qkv), _ptr(key_mask), _ptr(ctx), _ptr(lse), b, l, h,
                                     dropout_p, dropout_seed, _ptr(seed_ptr), _stream(qkv)), "cb_attention_fwd")
    return ctx, lse


def attention_bwd(qkv, key_mask, ctx, dctx, lse, b, l, h, dropout_p=0.0, dropout_seed=0, seed_ptr=None, out=None):
    dqkv = out if out is not None else torch.empty_like(qkv)
    ws = torch.empty(b * h * l, dtype=torch.float32, device=qkv.device)
    _chk(_lib.get().cb_attention_bwd(dtype_code(qkv.dtype), _ptr(qkv), _ptr(key_mask), _ptr(ctx), _ptr(dctx),
                                     _ptr(lse), _ptr(ws), _ptr(dqkv), b, l, h, dropout_p, dropout_seed, _ptr(seed_ptr),
                                     _stream(qkv)),
         "cb_attention_bwd")
    return dqkv


def cross_entropy(logits, labels, want_loss=True, dloss=None, want_grad=False, ignore_index=-100):
    """logits fp32 (rows, C), row stride may exceed C (padded vocab logits)."""
    rows, c = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    ld = logits.stride(0)
    loss = torch.empty(rows, dtype=torch.float32, device=logits.device) if want_loss else None
    dlogits = None
    if want_grad:
        dlogits = torch.empty_strided(logits.shape, logits.stride(), dtype=torch.float32, device=logits.device)
    _chk(_lib.get().cb_cross_entropy(_ptr(logits), ld, _ptr(labels), _ptr(loss), _ptr(dlogits), _ptr(dloss), rows, c,
                                     ignore_index, _stream(logits)), "cb_cross_entropy")
    return loss, dlogits


class MlmSelection:
    """What cb_mlm_select leaves on the device for one batch: the labelled text rows compacted into ``cap`` slots (see the header)."""
    __slots__ = ("cap", "rows", "lt", "l", "d", "v", "ignore_index", "slot_row", "slot_label", "tab", "rowmap", "counts", "loss_rows", "pred_rows")


def mlm_select(labels: torch.Tensor, lt: int, l: int, d: int, v: int, cap: int, counts: Optional[torch.Tensor] = None,
               ignore_index: int = -100) -> MlmSelection:
    """cb_mlm_select: labels int64 (B * Lt,) -> MlmSelection.  ``counts``: int64 (2,) = [count, dropped so far]; a new zeroed one when None
    (pass the same tensor again to keep the tally of drops).  One launch, no host sync."""
    assert labels.dtype == torch.int64 and labels.dim() == 1 and labels.is_contiguous()
    rows, dev = labels.numel(), labels.device
    s = MlmSelection()
    s.cap, s.rows, s.lt, s.l, s.d, s.v, s.ignore_index = cap, rows, lt, l, d, v, ignore_index
    s.slot_row = torch.empty(cap, dtype=torch.int32, device=dev)
    s.slot_label = torch.empty(cap, dtype=torch.int64, device=dev)
    s.tab = torch.empty(cap, dtype=torch.int64, device=dev)                    # cb_pixel entries
    s.rowmap = torch.empty(cap, dtype=torch.int32, device=dev)
    s.counts = counts if counts is not None else zeros(2, torch.int64, dev)
    assert s.counts.dtype == torch.int64 and s.counts.numel() == 2 and s.counts.is_contiguous()
    s.loss_rows = torch.empty(rows, dtype=torch.float32, device=dev)
    s.pred_rows = torch.empty(rows, dtype=torch.int64, device=dev)
    _chk(_lib.get().cb_mlm_select(_ptr(labels), ignore_index, rows, lt, l, d, v, cap, _ptr(s.slot_row), _ptr(s.slot_label), _ptr(s.tab),
                                  _ptr(s.rowmap), _ptr(s.counts), _ptr(s.loss_rows), _ptr(s.pred_rows), _stream(labels)), "cb_mlm_select")
    return s


def mlm_loss_fwd(logits: torch.Tensor, sel: MlmSelection) -> torch.Tensor:
    """cb_mlm_loss_fwd on the compact fp32 logits (cap, V) (row stride may exceed V): scatters the loss and the arg-max of every
    labelled slot into sel.loss_rows / sel.pred_rows and returns lse (cap,) for the backward (undefined at padding slots)."""
    cap, v = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and cap == sel.cap and v == sel.v
    lse = torch.empty(cap, dtype=torch.float32, device=logits.device)
    _chk(_lib.get().cb_mlm_loss_fwd(_ptr(logits), logits.stride(0), _ptr(sel.slot_row), _ptr(sel.slot_label), sel.ignore_index, cap, v,
                                    _ptr(lse), _ptr(sel.loss_rows), _ptr(sel.pred_rows), _stream(logits)), "cb_mlm_loss_fwd")
    return lse


def mlm_loss_bwd(logits: torch.Tensor, lse: torch.Tensor, sel: MlmSelection, dloss_rows: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """cb_mlm_loss_bwd: the (cap, V) view of a new (cap, ldd) ``dtype`` buffer (ldd = V rounded up to 16 bytes) holding d(loss)/d(logits)
    scaled by dloss_rows (B * Lt,) fp32 -- the A operand of the decoder's two backward GEMMs."""
    cap, v = logits.shape
    assert logits.dtype == torch.float32 and logits.stride(1) == 1 and cap == sel.cap and v == sel.v
    assert dloss_rows.dtype == torch.float32 and dloss_rows.is_contiguous() and dloss_rows.numel() == sel.rows
    per16 = 8 if dtype == torch.bfloat16 else 4
    ldd = (v + per16 - 1) // per16 * per16
    store = torch.empty(cap, ldd, dtype=dtype, device=logits.device)
    _chk(_lib.get().cb_mlm_loss_bwd(dtype_code(dtype), _ptr(logits), logits.stride(0), _ptr(lse), _ptr(sel.slot_row), _ptr(sel.slot_label),
                                    sel.ignore_index, _ptr(dloss_rows), _ptr(store), ldd, cap, v, _stream(logits)), "cb_mlm_loss_bwd")
    return store[:, :v]


def _vqa_args(logits, ans_ids, ans_scores):
    rows, c = logits.shape
    assert logits.dtype == torch.float32 and (logits.stride(1) == 1 or c == 1)
    assert ans_ids.dtype == torch.int32 and ans_scores.dtype == torch.float32 and ans_ids.dim() == 2 and ans_ids.shape == ans_scores.shape
    assert ans_ids.shape[0] == rows and ans_ids.is_contiguous() and ans_scores.is_contiguous(), (ans_ids.shape, rows)
    return rows, c, logits.stride(0) if rows > 1 else max(logits.stride(0), c), ans_ids.shape[1]


def vqa_loss_fwd(logits: torch.Tensor, ans_ids: torch.Tensor, ans_scores: torch.Tensor):
    """cb_vqa_loss_fwd on fp32 logits (rows, C) (row stride may exceed C) and the (rows, K) answer tables (int32 ids, padding < 0 or >= C;
    fp32 scores) -> (loss_rows fp32 (rows,): the row sums of the BCE-with-logits loss; pred_rows int64 (rows,): the arg-max;
    pred_score fp32 (rows,): the VQA soft accuracy of the arg-max)."""
    rows, c, ld, k = _vqa_args(logits, ans_ids, ans_scores)
    dev = logits.device
    loss = torch.empty(rows, dtype=torch.float32, device=dev)
    pred = torch.empty(rows, dtype=torch.int64, device=dev)
    score = torch.empty(rows, dtype=torch.float32, device=dev)
    _chk(_lib.get().cb_vqa_loss_fwd(_ptr(logits), ld, _ptr(ans_ids), _ptr(ans_scores), k, rows, c, _ptr(loss), _ptr(pred), _ptr(score),
                                    _stream(logits)), "cb_vqa_loss_fwd")
    return loss, pred, score


def vqa_loss_bwd(logits: torch.Tensor, ans_ids: torch.Tensor, ans_scores: torch.Tensor, dloss_rows: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """cb_vqa_loss_bwd: the (rows, C) view of a new (rows, ldd) ``dtype`` buffer (ldd = C rounded up to 16 bytes) holding
    d(sum_r dloss_rows[r] loss_rows[r])/d(logits) -- the A operand of the classifier's two backward GEMMs."""
    rows, c, ld, k = _vqa_args(logits, ans_ids, ans_scores)
    assert dloss_rows.dtype == torch.float32 and dloss_rows.is_contiguous() and dloss_rows.numel() == rows
    per16 = 8 if dtype == torch.bfloat16 else 4
    ldd = (c + per16 - 1) // per16 * per16
    store = torch.empty(rows, ldd, dtype=dtype, device=logits.device)
    _chk(_lib.get().cb_vqa_loss_bwd(dtype_code(dtype), _ptr(logits), ld, _ptr(ans_ids), _ptr(ans_scores), k, _ptr(dloss_rows), _ptr(store),
                                    ldd, rows, c, _stream(logits)), "cb_vqa_loss_bwd")
    return store[:, :c]


LOSS_MSE, LOSS_BCE, LOSS_RANK = 0, 1, 2


def head_loss(kind: int, x, y=None, want_loss=True, dloss=None, want_grad=False, group=1, margin=0.0):
    """cb_head_loss on contiguous fp32 logits: (loss, dx).  kind LOSS_RANK: x (rows, group), loss (rows, group - 1)."""
    assert x.dtype == torch.float32 and x.is_contiguous() and (y is None or (y.dtype == torch.float32 and y.is_contiguous() and y.numel() == x.numel()))
    n = x.numel()
    if kind == LOSS_RANK:
        lshape = (n // group, group - 1)
    else:
        lshape = tuple(x.shape)
    loss = torch.empty(lshape, dtype=torch.float32, device=x.device) if want_loss else None
    dx = torch.empty_like(x) if want_grad else None
    _chk(_lib.get().cb_head_loss(kind, _ptr(x), _ptr(y), _ptr(loss), _ptr(dloss), _ptr(dx), n, group, float(margin), _stream(x)), "cb_head_loss")
    return loss, dx


def retrieval_scores(logits, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(rows, 2) -> softmax[:, 1]; (rows, 1) or (rows,) -> sigmoid; fp32.  ``out``: a contiguous fp32 (rows,) slice on the logits' device
    to write in place (a piece of a score-matrix row); None = a fresh tensor."""
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    c = logits.shape[1] if logits.dim() == 2 else 1
    rows = logits.numel() // c
    if out is None:
        out = torch.empty(rows, dtype=torch.float32, device=logits.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (rows,) or not out.is_contiguous() or out.device != logits.device:
        raise ValueError(f"retrieval_scores: out must be {rows} contiguous fp32 values on {logits.device}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    _chk(_lib.get().cb_retrieval_scores(_ptr(logits), _ptr(out), rows, c, _stream(logits)), "cb_retrieval_scores")
    return out


RANK_ROW_QUERIES, RANK_COL_QUERIES = 0, 1          # CB_RANK_*: which axis of the video-major score matrix holds the queries


def retrieval_rank(scores: torch.Tensor, gt: torch.Tensor, axis: int, want_keys: bool = False):
    """cb_retrieval_rank on the fp32 video-major score matrix (n_videos, n_captions); the rows may be a view of a padded buffer (any dim-0
    stride >= n_captions, any 4-byte base), the last dimension is contiguous.  ``axis`` RANK_ROW_QUERIES: every row (video) is a query
    over its columns (video -> text); RANK_COL_QUERIES: every column (caption) is a query over the rows (text -> video).  ``gt``: int32,
    one ground-truth candidate index per query, on the same device.  -> rank int32 (n_queries,): the 1-based position of the ground truth
    in a stable descending sort of the keys rint(1e4 * score) (0 where gt is out of range); with ``want_keys`` -> (rank, keys int32
    (n_videos, n_captions)).  One launch, no host synchronisation."""
    if scores.dim() != 2 or scores.dtype != torch.float32:
        raise ValueError(f"retrieval_rank: expected an fp32 (n_videos, n_captions) matrix, got {scores.dtype} {tuple(scores.shape)}")
    n_rows, n_cols = scores.shape
    if n_cols > 1 and scores.stride(1) != 1:
        raise ValueError("retrieval_rank: the last dimension of the score matrix must be contiguous")
    ld = scores.stride(0) if n_rows > 1 else max(scores.stride(0), n_cols)
    if ld < n_cols:
        raise ValueError(f"retrieval_rank: the rows of the score matrix overlap (stride {ld} < {n_cols} columns)")
    axis = int(axis)
    n_q = n_cols if axis == RANK_COL_QUERIES else n_rows
    if gt.dtype != torch.int32 or gt.dim() != 1 or gt.numel() != n_q or not gt.is_contiguous() or gt.device != scores.device:
        raise ValueError(f"retrieval_rank: gt must be {n_q} contiguous int32 values on {scores.device}, got {gt.dtype} "
                         f"{tuple(gt.shape)} on {gt.device}")
    rank = torch.empty(n_q, dtype=torch.int32, device=scores.device)
    keys = torch.empty(n_rows, n_cols, dtype=torch.int32, device=scores.device) if want_keys else None
    _chk(_lib.get().cb_retrieval_rank(_ptr(scores), int(ld), n_rows, n_cols, axis, _ptr(gt), _ptr(rank), _ptr(keys), n_cols,
                                      _stream(scores)), "cb_retrieval_rank")
    return (rank, keys) if want_keys else rank


def mc_predict(stack: torch.Tensor, n_options: int, mode: int, clip_stride: Optional[int] = None):
    """cb_mc_predict on the fp32 stack (n_clips, R, C) of per-clip logits, R = n_q * n_options rows, C = 1 | 2; each clip contiguous, the
    dim-0 stride may exceed R * C (a view of a padded buffer; ``clip_stride`` overrides it, in elements) -> (scores fp32 (R,): the row's
    probability after pooling the clips with ``mode`` (AGG_MEAN | AGG_MAX | AGG_LSE); pred int32 (n_q,): the arg-max over each group of
    ``n_options`` rows).  One launch, no host synchronisation."""
    if stack.dim() != 3 or stack.dtype != torch.float32:
        raise ValueError(f"mc_predict: expected an fp32 (n_clips, rows, C) stack, got {stack.dtype} {tuple(stack.shape)}")
    n_clips, rows, c = stack.shape
    n_options = int(n_options)
    if n_options < 1 or rows % n_options != 0:
        raise ValueError(f"mc_predict: {rows} rows are not a multiple of n_options = {n_options}")
    if rows * c > 1 and not stack[0].is_contiguous():
        raise ValueError("mc_predict: each clip's (rows, C) logits must be contiguous")
    if clip_stride is None:
        clip_stride = stack.stride(0) if n_clips > 1 else max(stack.stride(0), rows * c)
    scores = torch.empty(rows, dtype=torch.float32, device=stack.device)
    pred = torch.empty(rows // n_options, dtype=torch.int32, device=stack.device)
    _chk(_lib.get().cb_mc_predict(_ptr(stack), int(clip_stride), n_clips, rows // n_options, n_options, c, int(mode), _ptr(scores), _ptr(pred),
                                  _stream(stack)), "cb_mc_predict")
    return scores, pred


QA_CLASSIFY, QA_COUNT = 0, 1


def qa_predict(stack: torch.Tensor, mode: int, kind: int = QA_CLASSIFY, labels: Optional[torch.Tensor] = None, want_pooled: bool = False,
               clip_stride: Optional[int] = None):
    """cb_qa_predict on the fp32 stack (n_clips, n_q, C) of per-clip logits; each clip contiguous, the dim-0 stride may exceed n_q * C (a
    view of a padded buffer; ``clip_stride`` overrides it, in elements) -> (pred int32 (n_q,), loss fp32 (n_q,) | None, pooled fp32
    (n_q, C) | None).  ``kind`` QA_CLASSIFY: pred = the arg-max over the classes of the logits pooled over the clips with ``mode``
    (AGG_MEAN | AGG_MAX | AGG_LSE), ``labels`` int32 (n_q,) class ids, loss = the mean over the clips of the per-clip cross entropy;
    QA_COUNT (C == 1): pred = clamp(trunc(pooled + 0.5), 1, 10), ``labels`` fp32 (n_q,), loss = the mean over the clips of the squared
    error.  Without ``labels`` there is no loss.  One launch, no host synchronisation."""
    if stack.dim() != 3 or stack.dtype != torch.float32:
        raise ValueError(f"qa_predict: expected an fp32 (n_clips, n_q, C) stack, got {stack.dtype} {tuple(stack.shape)}")
    n_clips, n_q, c = stack.shape
    if n_q * c > 1 and not stack[0].is_contiguous():
        raise ValueError("qa_predict: each clip's (n_q, C) logits must be contiguous")
    if labels is not None:
        want = torch.float32 if int(kind) == QA_COUNT else torch.int32
        if labels.dtype != want or labels.numel() != n_q or not labels.is_contiguous() or labels.device != stack.device:
            raise ValueError(f"qa_predict: labels must be {n_q} contiguous {want} values on {stack.device}, got {labels.dtype} "
                             f"{tuple(labels.shape)} on {labels.device}")
    if clip_stride is None:
        clip_stride = stack.stride(0) if n_clips > 1 else max(stack.stride(0), n_q * c)
    pred = torch.empty(n_q, dtype=torch.int32, device=stack.device)
    loss = torch.empty(n_q, dtype=torch.float32, device=stack.device) if labels is not None else None
    pooled = torch.empty(n_q, c, dtype=torch.float32, device=stack.device) if want_pooled else None
    _chk(_lib.get().cb_qa_predict(_ptr(stack), int(clip_stride), n_clips, n_q, c, int(mode), int(kind), _ptr(labels), _ptr(pred), _ptr(loss),
                                  _ptr(pooled), _stream(stack)), "cb_qa_predict")
    return pred, loss, pooled


def colsum(g, out, m=None, n=None, ldg=None):
    """out[n] += sum_m g[m, n] (fp32 atomics)."""
    m = g.shape[0] if m is None else m
    n = g.shape[1] if n is None else n
    _chk(_lib.get().cb_colsum(dtype_code(g.dtype), _ptr(g), ldg if ldg is not None else g.stride(0), _ptr(out), m, n,
                              _stream(g)), "cb_colsum")


def cast(src, dst):
    assert src.numel() == dst.numel()
    _chk(_lib.get().cb_cast(dtype_code(src.dtype), _ptr(src), dtype_code(dst.dtype), _ptr(dst), src.numel(),
                            _stream(src)), "cb_cast")
    return dst


def act_bwd(act, dy, ref):
    dx = torch.empty_like(dy)
    _chk(_lib.get().cb_act_bwd(dtype_code(dy.dtype), act, _ptr(dy), _ptr(ref), _ptr(dx), dy.numel(), _stream(dy)),
         "cb_act_bwd")
    return dx


def sq_sum(g, out, ws=None):
    """out += sum(g^2); with a scratch tensor ``ws`` (fp32, <= 1024 floats used) the result is independent of workgroup timing"""
    if g.dtype == torch.bfloat16:
        assert ws is not None, "bf16 gradients use the order-independent reduction (pass ws)"
        _chk(_lib.get().cb_sq_sum_det_bf16(_ptr(g), g.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream(g)), "cb_sq_sum_det_bf16")
    elif ws is not None:
        _chk(_lib.get().cb_sq_sum_det(_ptr(g), g.numel(), _ptr(out), _ptr(ws), ws.numel(), _stream(g)), "cb_sq_sum_det")
    else:
        _chk(_lib.get().cb_sq_sum(_ptr(g), g.numel(), _ptr(out), _stream(g)), "cb_sq_sum")


def sq_slot_count(M: int, N: int, batch: int = 1) -> int:
    """slots a cb_gemm call with ``sq_slots`` needs at most: one per 64 x 64 output tile and batch member"""
    return ((M + 63) // 64) * ((N + 63) // 64) * batch


def sq_sum_fold(g, segments, slots, out, ws):
    """out = sum of g[lo:hi]^2 over ``segments`` (<= 4 (lo, hi) element ranges) + sum(slots): the squared gradient norm of a step whose
    weight-gradient launches left their shares in ``slots`` (cb_sq_sum_fold; fixed order of addition)"""
    segs = [(int(lo), int(hi)) for lo, hi in segments if hi > lo]
    assert len(segs) <= 4
    arr = (C.c_int64 * (2 * max(1, len(segs))))(*[x for s in segs for x in s])
    _chk(_lib.get().cb_sq_sum_fold(_ptr(g), C.cast(arr, C.c_void_p), len(segs), _ptr(slots), slots.numel() if slots is not None else 0, _ptr(out), _ptr(ws),
                                   ws.numel(), _stream(out)), "cb_sq_sum_fold")


def adamw_hyper(lr, beta1, beta2, eps, weight_decay, step, max_norm=-1.0, grad_scale=1.0):
    """Host-side packing of the CB_HP_* array (see include/clipbert_hip.h)."""
    return [lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step, max_norm, grad_scale, 0.0, 0.0]


def adamw(p, g, m, v, w16, hyper_dev, grad_sq_sum=None):
    """hyper_dev: DEVICE fp32 tensor of >= HP_COUNT entries (adamw_hyper).  g: fp32, or bf16 (the reduced data-parallel wire image)."""
    if g.dtype == torch.bfloat16:
        _chk(_lib.get().cb_adamw_g16(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(w16), p.numel(), _ptr(hyper_dev), _ptr(grad_sq_sum),
                                     _stream(p)), "cb_adamw_g16")
        return
    _chk(_lib.get().cb_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(w16), p.numel(), _ptr(hyper_dev),
                             _ptr(grad_sq_sum), _stream(p)), "cb_adamw")


def optim_step(algo, p, g, m, v2, w16, hyper_dev, grad_sq_sum=None):
    """cb_optim_step: ``algo`` = _lib.OPT_ADAMW | OPT_ADAM | OPT_ADAMAX on one flat range; arguments as ``adamw`` (v2: exp_avg_sq, or Adamax's
    exp_inf).  g: fp32 or bf16."""
    _chk(_lib.get().cb_optim_step(algo, dtype_code(g.dtype), _ptr(p), _ptr(g), _ptr(m), _ptr(v2), _ptr(w16), p.numel(), _ptr(hyper_dev),
                                  _ptr(grad_sq_sum), _stream(p)), "cb_optim_step")


def dropout(x, p, seed=0, seed_ptr=None, out=None):
    y = torch.empty_like(x) if out is None else out
    _chk(_lib.get().cb_dropout(dtype_code(x.dtype), _ptr(x), _ptr(y), x.numel(), p, seed, _ptr(seed_ptr), _stream(x)),
         "cb_dropout")
    return y


def pixel_sample(lv: int, n: int, seed=0, seed_ptr=None, out=None, device=None):
    """cb_pixel_sample: int32 (n,) -- a uniformly random n-subset of range(lv) in ascending order, drawn on the device from ``seed`` plus the
    device word behind ``seed_ptr`` (the dropout convention).  One launch on the current stream of the output, no host sync: capturable.
    ``out``: int32, contiguous, at least n elements (its first n are written); else a new tensor on ``device`` (default: seed_ptr's)."""
    if out is None:
        if device is None:
            if seed_ptr is None:
                raise ValueError("pixel_sample: pass out=, device= or seed_ptr=")
            device = seed_ptr.device
        out = torch.empty(max(int(n), 0), dtype=torch.int32, device=device)
    assert out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= n, (out.dtype, out.shape, n)
    assert seed_ptr is None or (seed_ptr.dtype == torch.int64 and seed_ptr.numel() == 1 and seed_ptr.device == out.device)
    _chk(_lib.get().cb_pixel_sample(_ptr(out), lv, n, int(seed) % (1 << 64), _ptr(seed_ptr), _stream(out)), "cb_pixel_sample")
    return out[:n] if out.numel() != n else out


def mlm_mask(ids: torch.Tensor, p: float, seed=0, seed_ptr=None, special_ids=(101, 102), pad_id=0, mask_id=103, vocab_size=None,
             out_ids=None, out_labels=None, ignore_index: int = -100):
    """cb_mlm_mask: (ids_out, labels), both int64 of ids' shape -- the masked-LM masking of a padded (rows, Lt) id matrix, drawn on the
    device from ``seed`` plus the device word behind ``seed_ptr`` (the dropout convention; the definition is in the header).  ``ids`` is not
    written unless ``out_ids`` is ids itself.  ``special_ids``: at most 4 ids that are never labelled ([CLS], [SEP]); ``pad_id``: None or
    negative = no pad token; ``vocab_size``: the range of the random words, required.  One launch on the current stream of the outputs, no
    host sync: capturable."""
    if vocab_size is None:
        raise ValueError("mlm_mask: pass vocab_size= (the range of the random words)")
    assert ids.dtype == torch.int64 and ids.dim() == 2 and ids.is_contiguous(), (ids.dtype, ids.shape)
    ids_out = torch.empty_like(ids) if out_ids is None else out_ids
    labels = torch.empty_like(ids) if out_labels is None else out_labels
    for o in (ids_out, labels):
        assert o.dtype == torch.int64 and o.is_contiguous() and o.shape == ids.shape and o.device == ids.device, (o.dtype, o.shape, o.device)
    assert labels.data_ptr() != ids.data_ptr() and labels.data_ptr() != ids_out.data_ptr()
    assert seed_ptr is None or (seed_ptr.dtype == torch.int64 and seed_ptr.numel() == 1 and seed_ptr.device == ids_out.device)
    special = [int(x) for x in special_ids]
    arr = (C.c_int64 * max(len(special), 1))(*special)
    rows, lt = ids.shape
    _chk(_lib.get().cb_mlm_mask(_ptr(ids), rows, lt, arr, len(special), -1 if pad_id is None else int(pad_id), int(mask_id), int(vocab_size),
                                float(p), int(seed) % (1 << 64), _ptr(seed_ptr), _ptr(ids_out), _ptr(labels), ignore_index, _stream(ids_out)),
         "cb_mlm_mask")
    return ids_out, labels


def elu_bn1d_fwd(x, gamma, beta, running_mean, running_var, training: bool, momentum: float = 0.1, eps: float = 1e-5, save: bool = False):
    """ELU + BatchNorm1d over the batch (ClipBertForRegression.regressor[1:3]); returns (y, save_mean, save_invstd)."""
    b, d = x.shape
    y = torch.empty_like(x)
    sm = torch.empty(d, dtype=torch.float32, device=x.device) if save else None
    si = torch.empty(d, dtype=torch.float32, device=x.device) if save else None
    _chk(_lib.get().cb_elu_bn1d_fwd(dtype_code(x.dtype), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(y),
                                    _ptr(sm), _ptr(si), b, d, int(training), momentum, eps, _stream(x)), "cb_elu_bn1d_fwd")
    return y, sm, si


def elu_bn1d_bwd(dy, x, gamma, save_mean, save_invstd, dgamma, dbeta, training: bool):
    b, d = x.shape
    dx = torch.empty_like(x)
    _chk(_lib.get().cb_elu_bn1d_bwd(dtype_code(x.dtype), _ptr(dy), _ptr(x), _ptr(gamma), _ptr(save_mean), _ptr(save_invstd), _ptr(dx),
                                    _ptr(dgamma), _ptr(dbeta), b, d, int(training), _stream(x)), "cb_elu_bn1d_bwd")
    return dx


AGG_MEAN, AGG_MAX, AGG_LSE = 0, 1, 2


def clip_aggregate_fwd(stack: torch.Tensor, mode: int):
    """stack: (n_clips, ...) fp32 contiguous -> (out (...), argmax int32 | None)."""
    assert stack.dtype == torch.float32 and stack.is_contiguous()
    n = stack.shape[0]
    out = torch.empty(stack.shape[1:], dtype=torch.float32, device=stack.device)
    am = torch.empty(stack.shape[1:], dtype=torch.int32, device=stack.device) if mode == AGG_MAX else None
    _chk(_lib.get().cb_clip_aggregate_fwd(_ptr(stack), n, out.numel(), mode, _ptr(out), _ptr(am), _stream(stack)),
         "cb_clip_aggregate_fwd")
    return out, am


def clip_aggregate_bwd(dout: torch.Tensor, stack, out, argmax, n_clips: int, mode: int):
    dout = dout.contiguous()
    dx = torch.empty((n_clips,) + tuple(dout.shape), dtype=torch.float32, device=dout.device)
    _chk(_lib.get().cb_clip_aggregate_bwd(_ptr(dout), _ptr(stack), _ptr(out), _ptr(argmax), n_clips, dout.numel(), mode, _ptr(dx),
                                          _stream(dout)), "cb_clip_aggregate_bwd")
    return dx


def lse_loss(stack: torch.Tensor, labels: torch.Tensor, want_loss=True, dloss=None, want_grad=False):
    """stack: (n_clips, B, C) fp32 clip-major logits -> (loss (B,) | None, dlogits like stack | None)."""
    assert stack.dtype == torch.float32 and stack.is_contiguous() and stack.dim() == 3
    n, b, c = stack.shape
    loss = torch.empty(b, dtype=torch.float32, device=stack.device) if want_loss else None
    dx = torch.empty_like(stack) if want_grad else None
    _chk(_lib.get().cb_lse_loss(_ptr(stack), _ptr(labels.contiguous()), n, b, c, _ptr(loss), _ptr(dloss), _ptr(dx), _stream(stack)),
         "cb_lse_loss")
    return loss, dx
