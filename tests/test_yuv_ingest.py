"""cb_resize_pack_yuv420 (raw-frame ingest from the decoder's YUV 4:2:0 planes), data.collate_yuv_frames and RawFrames(pixfmt=...).

The entry point is DEFINED through cb_resize_pack_u8: its output equals, bit for bit, what cb_resize_pack_u8(hwc=0) writes for the uint8
RGB frames that tests/yuv_restatement.py (numpy float32, one rounding per written operation) makes of the planes.  Every comparison
with the kernel below is therefore an equality of bytes -- no tolerance.  The one bound of this file is CPU only and concerns the
restatement itself: against Pillow's YCbCr -> RGB (BT.601 full range, fixed-point tables) it may differ by one level per byte -- Pillow's
table entries are the coefficients rounded to 2^-16 steps and its sum is truncated, an error below one level; wrong signs, swapped
coefficients or swapped channels would show as tens of levels."""
import ctypes as C

import numpy as np
import pytest
import torch

import resize_restatement as R
import yuv_restatement as Y
from clipbert_amd import _lib, data, ops
from clipbert_amd import synthetic as S

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
LAYOUTS, MATRICES = ("i420", "nv12"), ("bt601", "bt601-full", "bt709", "bt709-full")
SIZE = 32
# (h, w, new_h, new_w) of one ragged batch launched at S = 32: odd sizes (the last chroma row / column serves ONE luma row / column),
# an identity-size frame, an upscaled and a downscaled (portrait) one
FRAMES = [(1, 1, 32, 32), (2, 3, 21, 32), (5, 7, 22, 32), (7, 5, 32, 22), (16, 16, 16, 16), (9, 20, 14, 32), (40, 24, 16, 9)]
assert all((nh, nw) == data.resize_size(h, w, 32) for h, w, nh, nw in FRAMES[:4] + FRAMES[5:6]) and FRAMES[6][2:] == data.resize_size(40, 24, 16)


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.uint8)


def _ragged(layout, matrix, seed=0, frames=FRAMES):
    """the batch as YUV frames (flat bytes, table) and as the planar RGB frames it stands for (flat bytes, table)"""
    yuv, rgb, t_yuv, t_rgb = [], [], [], []
    for k, (h, w, nh, nw) in enumerate(frames):
        planes = Y.random_planes(h, w, 100 * seed + k)
        t_yuv.append([sum(len(c) for c in yuv), h, w, nh, nw])
        t_rgb.append([sum(len(c) for c in rgb), h, w, nh, nw])
        yuv.append(Y.pack(*planes, layout))
        rgb.append(Y.planes_to_rgb(*planes, matrix).ravel())
        assert len(yuv[-1]) == Y.frame_bytes(h, w) == data.yuv420_frame_bytes(h, w)
    cat = lambda chunks: torch.from_numpy(np.concatenate(chunks))
    return cat(yuv), torch.tensor(t_yuv, dtype=torch.int64), cat(rgb), torch.tensor(t_rgb, dtype=torch.int64)


# ---- 1. kernel == definition -------------------------------------------------------------------------------------------------
def test_extreme_planes_fire_every_clamp():
    y, u, v = Y.random_planes(16, 16, 4)
    for matrix in MATRICES:
        rgb = Y.planes_to_rgb(y, u, v, matrix)
        assert all(rgb[c].min() == 0 and rgb[c].max() == 255 for c in range(3)), matrix


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("matrix", MATRICES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_equals_u8_kernel_on_restated_rgb(hw, layout, matrix, dtype):
    yuv, t_yuv, rgb, t_rgb = _ragged(layout, matrix)
    n = len(FRAMES)
    for pad in (0, 3):
        for extra_w in (0, 2):
            got = ops.resize_pack_yuv420(hw(yuv), hw(t_yuv), n, SIZE, dtype, MEAN, STD, layout=layout, matrix=matrix, pad=pad, extra_w=extra_w,
                                         host_table=t_yuv)
            ref = ops.resize_pack_u8(hw(rgb), hw(t_rgb), n, SIZE, dtype, MEAN, STD, hwc=False, pad=pad, extra_w=extra_w, host_table=t_rgb)
            assert got.shape == ref.shape == (n, SIZE + 2 * pad, SIZE + 2 * pad + extra_w, 4) and got.dtype == dtype
            differ = (_bytes(got) != _bytes(ref)).sum().item()
            assert differ == 0, f"{layout} {matrix} pad {pad} extra_w {extra_w}: {differ} bytes differ"


# ---- 2. the two layouts hold the same pictures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_layouts_agree(hw, dtype):
    n = len(FRAMES)
    for matrix in MATRICES:
        outs = []
        for layout in LAYOUTS:
            yuv, t_yuv, _, _ = _ragged(layout, matrix, seed=1)
            outs.append(ops.resize_pack_yuv420(hw(yuv), hw(t_yuv), n, SIZE, dtype, MEAN, STD, layout=layout, matrix=matrix, pad=3, extra_w=2))
        assert torch.equal(_bytes(outs[0]), _bytes(outs[1])), matrix


# ---- 3. the restatement against an independent implementation (CPU) --------------------------------------------------------------
def test_restatement_against_pillow():
    from PIL import Image
    rng = np.random.default_rng(3)
    ycc = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)                       # a 4:4:4 image: Y, Cb, Cr per pixel
    theirs = np.asarray(Image.frombytes("YCbCr", (64, 64), ycc.tobytes()).convert("RGB")).astype(np.int32)
    ours = Y.convert(ycc[..., 0], ycc[..., 1], ycc[..., 2], "bt601-full").transpose(1, 2, 0).astype(np.int32)
    diff = np.abs(ours - theirs)
    print(f"restatement vs Pillow (BT.601 full): max difference {diff.max()} level(s), {100 * (diff != 0).mean():.1f} % of the bytes differ")
    assert diff.max() <= 1


def test_restatement_layouts_and_odd_sizes():
    for h, w in ((1, 1), (5, 7), (6, 4)):
        planes = Y.random_planes(h, w, h * w)
        for layout in LAYOUTS:
            back = Y.unpack(Y.pack(*planes, layout), h, w, layout)
            assert all(np.array_equal(a, b) for a, b in zip(planes, back))
    y, u, v = Y.random_planes(5, 7, 9)
    rgb = Y.planes_to_rgb(y, u, v, "bt709")
    for i, j in ((4, 6), (4, 0), (3, 6), (2, 5)):                                   # pixel (i, j) uses chroma sample (i >> 1, j >> 1)
        one = Y.convert(y[i:i + 1, j:j + 1], u[i >> 1:(i >> 1) + 1, j >> 1:(j >> 1) + 1], v[i >> 1:(i >> 1) + 1, j >> 1:(j >> 1) + 1], "bt709")
        assert np.array_equal(one[:, 0, 0], rgb[:, i, j])


# ---- 4. bad rows and arguments -----------------------------------------------------------------------------------------------
THREE = [(6, 10, 19, 32), (7, 9, 24, 32), (8, 8, 32, 32)]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_bad_rows_become_padding_and_neighbours_stay(hw, layout):
    yuv, table, _, _ = _ragged(layout, "bt601", seed=2, frames=THREE)
    nbytes, mid = yuv.numel(), Y.frame_bytes(7, 9)
    call = lambda t, host=None, S=SIZE: ops.resize_pack_yuv420(hw(yuv), hw(t), 3, S, torch.float32, MEAN, STD, layout=layout, pad=3, extra_w=2,
                                                               host_table=host).cpu()
    good = call(table, table)
    pad_only = R.packed_reference(torch.zeros(1, 3, SIZE, SIZE), [(0, 0)], MEAN, STD, 3, 2)[0][0]      # ImagePad's zero pixel, normalised
    assert not torch.equal(good[1], pad_only)
    # a frame fits when it ends exactly at the buffer's end; one byte further it does not (h * w + 2 * ch * cw bytes: 103 for 7 x 9, not 63 * 3 / 2)
    assert table[2, 0] + Y.frame_bytes(8, 8) == nbytes and mid == 103
    last = table.clone()
    last[1] = torch.tensor([nbytes - mid, 7, 9, 24, 32])
    assert not torch.equal(call(last, last)[1], pad_only)
    off = int(table[1, 0])
    bad_rows = [([nbytes - mid + 1, 7, 9, 24, 32], "leaves the"), ([-1, 7, 9, 24, 32], "leaves the"), ([off, 4000, 4000, 24, 32], "leaves the"),
                ([off, 0, 9, 24, 32], "is 0 x 9"), ([off, 7, -3, 24, 32], "is 7 x -3"), ([off, 7, 9, 24, SIZE + 1], "resizes to"),
                ([off, 7, 9, 0, 32], "resizes to")]
    for row, message in bad_rows:
        bad = table.clone()
        bad[1] = torch.tensor(row)
        out = call(bad)                                                       # no host table: guarded on the device, nothing is read
        assert torch.equal(out[1], pad_only), row
        assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2]), row
        with pytest.raises(RuntimeError, match=f"cb_resize_pack_yuv420: frame 1 .*{message}"):
            call(bad, bad)                                                    # with one: refused before the launch, the frame named


def test_bad_codes_launch_nothing(hw):
    yuv, table, _, _ = _ragged("i420", "bt601", frames=THREE)
    yuv, table = hw(yuv), hw(table)
    dst = hw(torch.full((3, SIZE, SIZE, 4), 7.0))
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    fn = _lib.get().cb_resize_pack_yuv420
    call = lambda dtype=_lib.CB_F32, layout=0, matrix=0, n=3: fn(dtype, ops._ptr(yuv), yuv.numel(), ops._ptr(table), None, n, layout, matrix, mean, std,
                                                               ops._ptr(dst), SIZE, SIZE, SIZE, 0, ops._stream(yuv))
    for kw, message in ((dict(layout=2), "bad layout"), (dict(layout=-1), "bad layout"), (dict(matrix=4), "bad matrix"), (dict(matrix=-1), "bad matrix"),
                        (dict(dtype=2), "bad dtype"), (dict(n=0), "bad N"), (dict(n=65536), "bad N")):
        assert call(**kw) != 0 and message in _lib.get().cb_last_error().decode(), kw
    assert torch.count_nonzero(dst.cpu() != 7.0) == 0
    assert call() == 0 and torch.count_nonzero(dst.cpu() == 7.0) == 0
    with pytest.raises(KeyError):
        ops.resize_pack_yuv420(yuv, table, 3, SIZE, torch.float32, MEAN, STD, layout="yv12")
    assert _lib.get().cb_version() >= 10


def test_refuses_cpu_tensors_on_the_product_path():
    yuv, table, _, _ = _ragged("i420", "bt601", frames=THREE)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.resize_pack_yuv420(yuv, table, 3, SIZE, torch.float32, MEAN, STD)


# ---- 5. RawFrames plumbing ------------------------------------------------------------------------------------------------------
VIDEO_SHAPES = [(4, 45, 79), (4, 91, 61)]                       # (T, h, w): odd sizes, landscape and portrait


def _yuv_videos(layout, shapes=VIDEO_SHAPES, seed=21):
    """[(frames_u8 (T, frame_bytes), h, w)] and the planes they were packed from"""
    videos, planes = [], []
    for i, (t, h, w) in enumerate(shapes):
        p = [Y.random_planes(h, w, 1000 * seed + 10 * i + k) for k in range(t)]
        videos.append((torch.from_numpy(np.stack([Y.pack(*f, layout) for f in p])), h, w))
        planes.append(p)
    return videos, planes


def _rgb_videos(planes, matrix):
    """the planar uint8 RGB videos (T, 3, h, w) the planes stand for"""
    return [torch.from_numpy(np.stack([Y.planes_to_rgb(*f, matrix) for f in p])) for p in planes]


def test_collate_yuv_frames_rows_and_offsets():
    videos, _ = _yuv_videos("i420", shapes=[(2, 5, 7), (2, 9, 4)])
    rf = data.collate_yuv_frames(videos, 16, layout="i420", matrix="bt709")
    assert (5 * 7 + 2 * 3 * 4, 9 * 4 + 2 * 5 * 2) == (59, 56)
    assert rf.table.tolist() == [[[0, 5, 7, 11, 16], [59, 5, 7, 11, 16]], [[118, 9, 4, 16, 7], [174, 9, 4, 16, 7]]]
    assert rf.flat.numel() == 2 * 59 + 2 * 56 and rf.shape == (2, 2, 3, 16, 16) and rf.pixfmt == "i420" and rf.matrix == "bt709"
    assert torch.equal(rf.flat[118:174], videos[1][0][0]) and rf.host_table is rf.table
    with pytest.raises(AssertionError):
        data.collate_yuv_frames([(videos[0][0], 5, 8)], 16)                       # 5 x 8 frames have 60 bytes
    with pytest.raises(AssertionError):
        data.collate_yuv_frames(videos, 16, layout="yv12")
    with pytest.raises(AssertionError):
        data.collate_yuv_frames([videos[0], (videos[1][0][:1], 9, 4)], 16)        # different frame counts
    with pytest.raises(ValueError):
        data.collate_yuv_frames([(torch.zeros(1, 800 + 2 * 200, dtype=torch.uint8), 400, 2)], 32)     # 400 x 2 -> 32 x 0, as collate_raw_frames


def test_pixfmt_and_matrix_travel_with_raw_frames():
    plain = data.collate_raw_frames([torch.zeros(2, 4, 6, 3, dtype=torch.uint8)], 8)
    assert (plain.pixfmt, plain.matrix, plain.hwc) == ("rgb", "bt601", True)
    assert data.RawFrames(plain.flat, plain.table, 8).pixfmt == "rgb" and "hwc=True" in repr(plain)
    assert plain.to("cpu").pixfmt == "rgb" and plain[0:1].view(2, 1, 3, 8, 8).pixfmt == "rgb"
    videos, _ = _yuv_videos("nv12", shapes=[(4, 5, 7), (4, 9, 4), (4, 6, 6)])
    rf = data.collate_yuv_frames(videos, 16, layout="nv12", matrix="bt709-full")
    tail = (3, 16, 16)
    derived = [rf.view(6, 2, *tail), rf.reshape(12, 1, *tail), rf.view(3, 2, 2, *tail).transpose(0, 1), rf.view(3, 2, 2, *tail)[:, 1].contiguous(),
               rf[1:3], rf[2], rf[0:1, 1:3], rf.contiguous(), rf.to("cpu"), rf.view(3, 2, 2, *tail).transpose(0, 1).reshape(6, 2, *tail)]
    for i, d in enumerate(derived):
        assert isinstance(d, data.RawFrames) and (d.pixfmt, d.matrix, d.max_img_size) == ("nv12", "bt709-full", 16), i
        assert d.flat.data_ptr() == rf.flat.data_ptr()
    assert "nv12" in repr(rf) and "bt709-full" in repr(rf)
    batches = [dict(visual_inputs=rf, nested=[rf[0:1]], k=i) for i in range(3)]
    for i, b in enumerate(data.PrefetchLoader(batches, device="cpu")):
        for got, want in ((b["visual_inputs"], rf), (b["nested"][0], rf[0:1])):
            assert isinstance(got, data.RawFrames) and (got.pixfmt, got.matrix, got.max_img_size) == ("nv12", "bt709-full", 16)
            assert torch.equal(got.flat, want.flat) and torch.equal(got.table, want.table) and torch.equal(got.host_table, want.host_table)
        assert b["k"] == i
    with pytest.raises(AssertionError):
        data.RawFrames(rf.flat, rf.table, 16, pixfmt="yv12")


@pytest.mark.gpu
def test_prefetch_loader_stages_yuv_frames_to_the_gpu():
    videos, _ = _yuv_videos("i420", shapes=[(2, 5, 7), (2, 9, 4)])
    rf = data.collate_yuv_frames(videos, 16, matrix="bt601-full")
    for b in data.PrefetchLoader([dict(visual_inputs=rf)] * 3, device="cuda:0"):
        got = b["visual_inputs"]
        assert got.flat.is_cuda and got.table.is_cuda and (got.pixfmt, got.matrix) == ("i420", "bt601-full")
        assert torch.equal(got.flat.cpu(), rf.flat) and torch.equal(got.table.cpu(), rf.table) and torch.equal(got.host_table, rf.table)


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------
RET = dict(num_labels=2, loss_type="ce", margin=0.1)
MODEL_SIZE = 64


def _model_inputs(cfg, layout, matrix):
    videos, planes = _yuv_videos(layout)
    yuv = data.collate_yuv_frames(videos, MODEL_SIZE, layout=layout, matrix=matrix)
    rgb = data.collate_raw_frames(_rgb_videos(planes, matrix), MODEL_SIZE, hwc=False)
    assert yuv.shape == rgb.shape and 2 * yuv.flat.numel() < rgb.flat.numel() + 4 * 8 * 100         # half the bytes (odd sizes round up)
    ids, mask = S.synthetic_text(4, 6, 5, cfg["vocab_size"])
    return yuv, rgb, ids.clamp(max=cfg["vocab_size"] - 1), mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout,matrix", [("i420", "bt601"), ("nv12", "bt709-full")])
def test_model_on_yuv_frames_equals_model_on_restated_rgb(hw, dtype, layout, matrix):
    from test_model_small import build, to_dev
    cfg, sd, model = build("retrieval", RET, dtype, hw.dev)
    yuv, rgb, ids, mask = _model_inputs(cfg, layout, matrix)
    common = to_dev(dict(text_input_ids=ids, text_input_mask=mask, labels=torch.tensor([1, 0, 1, 0])), hw.dev)
    with torch.no_grad():
        a = model(dict(common, visual_inputs=yuv.to(hw.dev), n_examples_list=[2, 2]))
        b = model(dict(common, visual_inputs=rgb.to(hw.dev), n_examples_list=[2, 2]))
        ga, gb = model.grid_features(yuv.to(hw.dev)), model.grid_features(rgb.to(hw.dev))
    assert torch.equal(_bytes(ga), _bytes(gb))
    assert torch.equal(_bytes(a["logits"]), _bytes(b["logits"])) and torch.equal(_bytes(a["loss"]), _bytes(b["loss"]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_step_on_yuv_frames_equals_train_step_on_restated_rgb(hw, dtype):
    from types import SimpleNamespace
    from clipbert_amd import optim, tasks
    from test_model_small import build, to_dev
    tcfg = SimpleNamespace(train_n_clips=2, num_frm=2, score_agg_func="mean", learning_rate=1e-3, cnn_learning_rate=1e-3, decay="linear",
                           cnn_lr_decay="linear", num_train_steps=10, warmup_ratio=0.1, transformer_lr_mul=1.0, cnn_lr_mul=1.0)
    losses = []
    for kind in ("yuv", "rgb"):                                  # two models from the same seed, one step each
        torch.manual_seed(0)
        cfg, sd, model = build("retrieval", RET, dtype, hw.dev)
        model.train()
        opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
        yuv, rgb, ids, mask = _model_inputs(cfg, "i420", "bt601")
        batch = dict(to_dev(dict(text_input_ids=ids, text_input_mask=mask, labels=torch.tensor([1, 0, 1, 0])), hw.dev),
                     visual_inputs=(yuv if kind == "yuv" else rgb).to(hw.dev), n_examples_list=[2, 2])
        watched = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters() if n.endswith("res5.2.conv3.weight")}
        losses.append(tasks.train_step(model, opt, batch, tcfg, global_step=0).float().cpu())
        assert torch.isfinite(losses[-1]).all() and len(watched) == 1
        for n, p in model.named_parameters():
            if n in watched:
                assert not torch.equal(p.detach().float().cpu(), watched[n]), n           # the step reached the CNN
    assert torch.equal(losses[0], losses[1]), (losses[0], losses[1])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_launch_is_graph_capturable(layout):
    """No host synchronisation, geometry read on the device: the launch is captured once; new bytes and a new table of the same (N, S)
    are then written into the captured buffers in place, and the replay must give what an eager launch gives on them."""
    dev = torch.device("cuda", 0)
    first, _ = _yuv_videos(layout, shapes=[(2, 45, 79), (2, 91, 61)], seed=5)
    second, _ = _yuv_videos(layout, shapes=[(2, 91, 61), (2, 45, 79)], seed=6)
    a, b = (data.collate_yuv_frames(v, MODEL_SIZE, layout=layout) for v in (first, second))
    assert a.flat.numel() == b.flat.numel() and not torch.equal(a.table, b.table)
    flat, table = a.flat.to(dev), a.table.view(-1, 5).to(dev)
    run = lambda f, t: ops.resize_pack_yuv420(f, t, 4, MODEL_SIZE, torch.bfloat16, MEAN, STD, layout=layout, pad=3, extra_w=2)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eager_first = run(flat, table).clone()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run(flat, table)
    flat.copy_(b.flat.to(dev))
    table.copy_(b.table.view(-1, 5).to(dev))
    graph.replay()
    torch.cuda.synchronize()
    eager_second = run(b.flat.to(dev), b.table.view(-1, 5).to(dev))
    assert torch.equal(_bytes(out), _bytes(eager_second)) and not torch.equal(_bytes(out), _bytes(eager_first))
