"""cb_resize_pack_u8 (raw-frame ingest): native-resolution uint8 frames -> the reference's ImageResize + ImagePad + ImageNorm, packed
for the stem.  Yardstick: the torch restatement of tests/resize_restatement.py, pinned to the reference's own classes by the live CPU
test below and by the recorded fixture tests/golden/resize_pad_small.npz (tools/make_resize_golden.py).

Bounds (none of them measured on the kernel):
* fp32 interior, on the pre-normalisation 0..255 scale: 1e-4.  Kernel and F.interpolate share the coordinate arithmetic exactly; what is
  left is the order / fusing of the blend's <= 4 roundings at <= 255 (4 x 2^-17 = 3e-5) on either side.
* padding band: EXACTLY (0 - mean) * (1 / std); halo and the 4th channel: exactly 0.
* bf16: within 1 bf16 ulp of the restatement rounded to bf16 everywhere, and at most 1 % of the interior elements different at all
  (a 3e-5 difference before the rounding can only flip a value that sits on a rounding boundary)."""
import numbers
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_restatement as R
from clipbert_amd import data, ops
from oracle import ref_shim

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "resize_pad_small.npz")
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
live = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")


# ---- 1. restatement == reference (CPU, live) --------------------------------------------------------------------------------
@live
def test_restatement_equals_reference_live():
    from torch.nn.modules.utils import _quadruple
    from oracle import ref_functions as RF
    ns = RF.load(RF.DATA_UTILS, ["get_padding", "ImagePad", "get_resize_size", "ImageResize"],
                 extra_ns=dict(Image=SimpleNamespace(BILINEAR=2), img_tensor_resize=F.interpolate, img_tensor_pad=F.pad, _quadruple=_quadruple,
                               numbers=numbers, img_resize=None, img_pad=None))
    ImageNorm = RF.image_norm_class()
    for i, ((t, h, w), S) in enumerate(R.PIN_CASES):
        v = R.random_video(t, h, w, 40 + i)
        ref_size = ns["get_resize_size"](v, S)
        assert tuple(ref_size) == R.resize_size(h, w, S) == data.resize_size(h, w, S), (h, w, S)
        ref = ns["ImagePad"](S, S)(ns["ImageResize"](S, "bilinear")(v.float()))
        ours = R.resize_pad(v, S)
        assert ours.shape == ref.shape == (t, 3, S, S)
        assert torch.equal(ours, ref), (h, w, S, (ours - ref).abs().max().item())
        for mean, std in ((MEAN, STD), (MEAN, (1.0, 1.0, 1.0))):
            ref_n = ImageNorm(mean=mean, std=std)(ref.clone().unsqueeze(0))
            assert torch.equal(R.image_norm(ours.unsqueeze(0), mean, std), ref_n)
    assert data.resize_size(333, 500, 768) == (511, 768)            # int() truncates 511.488; a rounded ratio would give 512
    for h, w in ((100, 501), (501, 100), (100, 500), (64, 64)):
        is_extreme = RF.load_method(os.path.join("src", "datasets", "dataset_base.py"), "ClipBertBaseDataset", "_is_extreme_aspect_ratio")
        assert data.is_extreme_aspect_ratio(h, w) == is_extreme(None, torch.empty(1, 3, h, w), max_ratio=5.)


def test_resize_size_truncates():
    assert data.resize_size(333, 500, 768) == (511, 768) == R.resize_size(333, 500, 768)
    assert data.resize_size(100, 180, 224) == (124, 224) and data.resize_size(480, 360, 448) == (448, 336)
    assert data.resize_size(64, 64, 64) == (64, 64)
    assert data.is_extreme_aspect_ratio(100, 501) and data.is_extreme_aspect_ratio(501, 100) and not data.is_extreme_aspect_ratio(100, 500)


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _run_kernel(hw, videos, S, dtype, mean, std, hwc, extra_w=2):
    """planar uint8 videos -> (packed output on the CPU, new sizes per frame) through collate_raw_frames + ops.resize_pack_u8"""
    videos = [f.unsqueeze(0) for v in videos for f in v]             # (the videos differ in length here: one single-frame video per frame)
    vids = [v.permute(0, 2, 3, 1).contiguous() for v in videos] if hwc else videos
    rf = data.collate_raw_frames(vids, S, hwc=hwc).to(hw.dev)
    table, host = rf.packed_table()
    out = ops.resize_pack_u8(rf.flat, table, rf.n_frames, S, dtype, mean, std, hwc=hwc, pad=3, extra_w=extra_w, host_table=host)
    sizes = [data.resize_size(v.shape[2], v.shape[3], S) for v in videos for _ in range(v.shape[0])]
    return out.cpu(), sizes


def _check_fp32(out, padded, sizes, mean, std, extra_w=2, bound=1e-4):
    ref, interior = R.packed_reference(padded, sizes, mean, std, 3, extra_w)
    S = padded.shape[-1]
    assert out.shape == ref.shape and out.dtype == torch.float32
    std_bgr = torch.tensor([std[2], std[1], std[0]], dtype=torch.float64)
    err = (out[:, 3:3 + S, 3:3 + S, :3].double() - ref[:, 3:3 + S, 3:3 + S, :3].double()).abs() * std_bgr      # 0..255 scale
    worst = err[interior].max().item()
    print(f"resize_pack fp32: worst interior error {worst:.3e} on the 0..255 scale (bound {bound:.0e})")
    assert worst <= bound, worst
    band = torch.zeros_like(out, dtype=torch.bool)
    band[:, 3:3 + S, 3:3 + S, :3] = ~interior.unsqueeze(-1)
    assert torch.equal(out[band], ref[band])                                    # ImagePad's zero pixel, normalised: exact
    band[:, 3:3 + S, 3:3 + S, :3] = True
    assert torch.count_nonzero(out[~band]) == 0                                 # halo, extra columns, 4th channel: exact zeros
    return worst


RAGGED = {64: [(2, 48, 80), (1, 90, 60), (2, 64, 64), (1, 33, 50)], 224: [(1, 240, 320), (2, 100, 180), (1, 360, 270)]}


# ---- 2. kernel vs restatement, fp32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", [True, False])
@pytest.mark.parametrize("S", [64, 224])
def test_ragged_batch_fp32(hw, S, hwc):
    videos = [R.random_video(t, h, w, 7 * S + i) for i, (t, h, w) in enumerate(RAGGED[S])]
    out, sizes = _run_kernel(hw, videos, S, torch.float32, MEAN, STD, hwc)
    padded = torch.cat([R.resize_pad(v, S) for v in videos])
    _check_fp32(out, padded, sizes, MEAN, STD)


# ---- 3. kernel vs restatement, bf16 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", [True, False])
@pytest.mark.parametrize("S", [64, 224])
def test_ragged_batch_bf16(hw, S, hwc):
    videos = [R.random_video(t, h, w, 11 * S + i) for i, (t, h, w) in enumerate(RAGGED[S])]
    out, sizes = _run_kernel(hw, videos, S, torch.bfloat16, MEAN, STD, hwc)
    padded = torch.cat([R.resize_pad(v, S) for v in videos])
    ref32, interior = R.packed_reference(padded, sizes, MEAN, STD, 3, 2)
    ref = ref32.to(torch.bfloat16)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    # distance in bf16 ulps through the ordered integer image of the bit patterns (sign-magnitude -> two's complement)
    def ordered(t):
        bits = t.view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7fff), bits)
    ulps = (ordered(out) - ordered(ref)).abs()
    assert ulps.max().item() <= 1, f"{ulps.max().item()} bf16 ulps"
    inner = interior.unsqueeze(-1).expand(-1, -1, -1, 3)
    differ = (ulps[:, 3:3 + S, 3:3 + S, :3][inner] != 0).float().mean().item()
    print(f"resize_pack bf16: {differ:.3e} of the interior elements differ from the rounded restatement (bound 1e-2)")
    assert differ <= 0.01, f"share of interior elements that differ from the rounded restatement: {differ:.3e}"
    outside = torch.ones_like(ulps, dtype=torch.bool)
    outside[:, 3:3 + S, 3:3 + S, :3] = ~inner
    assert torch.equal(out[outside], ref[outside])                              # padding band exact, halo / 4th channel zero


# ---- 4. identity: frames that already are S x S == cb_stem_pack(src_u8 = 1), bit for bit ---------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hwc", [True, False])
def test_identity_equals_stem_pack(hw, dtype, hwc):
    S = 64
    videos = [R.random_video(2, S, S, 3), R.random_video(2, S, S, 4)]
    out, _ = _run_kernel(hw, videos, S, dtype, MEAN, STD, hwc)
    ref = ops.stem_pack(hw(torch.cat(videos).contiguous()), dtype, 3, MEAN, STD, extra_w=2).cpu()
    assert out.shape == ref.shape and torch.equal(out.view(torch.uint8), ref.view(torch.uint8))


# ---- 5. the reference's recorded output ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", [True, False])
def test_recorded_reference_fixture(hw, hwc):
    assert os.path.getsize(GOLDEN) < 200 * 1024
    z = np.load(GOLDEN)
    S = int(z["max_img_size"])
    videos = [torch.from_numpy(z[f"video{i}"]) for i in range(3)]
    padded = torch.cat([torch.from_numpy(z[f"padded{i}"]) for i in range(3)])
    assert len({v.shape[2:] for v in videos}) == 3
    out, sizes = _run_kernel(hw, videos, S, torch.float32, MEAN, STD, hwc)
    _check_fp32(out, padded, sizes, MEAN, STD)
    assert torch.equal(torch.cat([R.resize_pad(v, S) for v in videos]), padded)     # ... and the restatement reproduces the record


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked(hw):
    S = 32
    rf = data.collate_raw_frames([R.random_video(1, 20, 30, 1)], S, hwc=False).to(hw.dev)
    table, host = rf.packed_table()
    call = lambda **kw: ops.resize_pack_u8(rf.flat, kw.get("table", table), 1, kw.get("S", S), torch.float32, MEAN, STD, hwc=False,
                                           host_table=kw.get("host", host))
    call()
    with pytest.raises(RuntimeError, match="resizes to"):
        call(S=16)                                                           # new_w = 32 > S
    bad = host.clone()
    bad[0, 0] = 1                                                            # one byte past the buffer's end
    with pytest.raises(RuntimeError, match="leaves the"):
        call(host=bad)
    bad = host.clone()
    bad[0, 1] = 0
    with pytest.raises(RuntimeError, match="frame 0 is"):
        call(host=bad)
    # the kernel itself never reads through a row that does not fit the buffer: such a frame comes out as padding only
    out = call(table=hw(torch.tensor([[0, 4000, 4000, 32, 32]], dtype=torch.int64)), host=None).cpu()
    ref, _ = R.packed_reference(torch.zeros(1, 3, S, S), [(0, 0)], MEAN, STD, 3, 0)
    assert torch.equal(out, ref)


def test_refuses_cpu_tensors_on_the_product_path():
    rf = data.collate_raw_frames([R.random_video(1, 20, 30, 1)], 32, hwc=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_pack_u8(rf.flat, rf.table.view(1, 5), 1, 32, torch.float32, MEAN, STD, hwc=False)
