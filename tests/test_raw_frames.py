"""data.RawFrames -- the ragged batch of native-resolution uint8 frames -- through the host container operations the task loops apply
to batch["visual_inputs"], through PrefetchLoader, and through the model: ClipBert on a RawFrames batch against the same model on the
reference's resized + padded + normalised fp32 tensor (tests/resize_restatement.py, pinned to the reference in test_resize_pack.py).

Model-level bounds are the ones tests/test_model_small.py applies to this small model: 1e-3 on fp32 logits (its fp32 parity tolerance
on the GPU), 5e-2 on bf16 logits (test_bf16_mode_close).  The two inputs differ by fp32 round-off on the image (<= 1e-4 of 255)."""
from types import SimpleNamespace

import pytest
import torch

import resize_restatement as R
from clipbert_amd import data, optim, tasks
from clipbert_amd import synthetic as S
from test_model_small import build, to_dev

RET = dict(num_labels=2, loss_type="ce", margin=0.1)
SIZE = 64
SHAPES = [(4, 48, 80), (4, 90, 60)]                 # (T, h, w) per video: landscape and portrait, both resampled to fit 64 x 64
LOGIT_BOUND = {torch.float32: 1e-3, torch.bfloat16: 5e-2}


def _videos(seed=21, shapes=SHAPES):
    return [R.random_video(t, h, w, seed + i) for i, (t, h, w) in enumerate(shapes)]


def _raw(videos, hwc=True, size=SIZE):
    return data.collate_raw_frames([v.permute(0, 2, 3, 1).contiguous() for v in videos] if hwc else videos, size, hwc=hwc)


def _densify(rf: data.RawFrames) -> torch.Tensor:
    """the fp32 tensor a RawFrames stands for (before ImageNorm), frame by frame through the restatement"""
    rows = rf.host_table.reshape(-1, 5).tolist()
    flat = rf.flat.cpu()
    out = []
    for off, h, w, nh, nw in rows:
        px = flat[off:off + 3 * h * w]
        frame = px.view(h, w, 3).permute(2, 0, 1) if rf.hwc else px.view(3, h, w)
        assert (nh, nw) == R.resize_size(h, w, rf.max_img_size)
        out.append(R.resize_pad(frame.unsqueeze(0).contiguous(), rf.max_img_size)[0])
    return torch.stack(out).view(rf.shape)


# ---- 7. host container ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hwc", [True, False])
def test_container_ops_equal_tensor_ops(hwc):
    videos = _videos(shapes=[(4, 20, 36), (4, 40, 24), (4, 32, 32)])
    rf = _raw(videos, hwc, size=32)
    dense = R.dense_batch(videos, 32)                                             # (3, 4, 3, 32, 32)
    assert rf.shape == dense.shape and rf.device == dense.device and rf.dim() == 5 and len(rf) == 3 and rf.n_frames == 12
    assert torch.equal(_densify(rf), dense)
    flat_ptr = rf.flat.data_ptr()
    ops = [lambda v: v.view(3 * 2, 2, *v.shape[2:]),                               # forward_clips_stack(fold=True)
           lambda v: v.view(3, 2, 2, *v.shape[2:])[:, 1].contiguous(),             # ... fold=False: clip c of every video
           lambda v: v.view(3, 2, 2, *v.shape[2:])[:, 0],
           lambda v: v[1:3], lambda v: v[2], lambda v: v[0:1, 1:3],
           lambda v: v[1:2].view(2, 2, *v.shape[2:])[1:2],                         # inference_retrieval_video: clips of one video
           lambda v: v.view(3, 2, 2, *v.shape[2:]).transpose(0, 1).reshape(6, 2, *v.shape[2:]).contiguous(),      # qa_predict(fold_clips)
           lambda v: v.reshape(12, 1, *v.shape[2:])]
    for i, op in enumerate(ops):
        a, b = op(rf), op(dense)
        assert isinstance(a, data.RawFrames) and a.shape == b.shape, i
        assert torch.equal(_densify(a), b), i
        assert a.flat.data_ptr() == flat_ptr                                      # pixel bytes are shared, never copied
    assert not rf.view(3, 2, 2, 3, 32, 32)[:, 1].is_contiguous() and rf.view(3, 2, 2, 3, 32, 32)[:, 1].contiguous().is_contiguous()
    with pytest.raises(ValueError):
        rf.view(3, 4, 3, 16, 64)                                                  # only the batch dimensions regroup
    with pytest.raises(IndexError):
        rf[:, :, 0]
    moved = rf.to("cpu")
    assert moved.shape == rf.shape and torch.equal(_densify(moved), dense)
    t, ht = rf[:, 1:3].packed_table()
    assert t.shape == (6, 5) and t.is_contiguous() and torch.equal(t, ht)


def test_collate_checks_its_input():
    v = R.random_video(2, 20, 36, 1)
    with pytest.raises(AssertionError):
        data.collate_raw_frames([v, R.random_video(3, 20, 36, 2)], 32, hwc=False)          # different frame counts
    with pytest.raises(AssertionError):
        data.collate_raw_frames([v], 32, hwc=True)                                         # planar frames announced as interleaved
    with pytest.raises(ValueError):
        data.collate_raw_frames([R.random_video(1, 400, 2, 3)], 32, hwc=False)             # 400 x 2 -> 32 x 0
    rf = data.collate_raw_frames([v, R.random_video(2, 40, 24, 2)], 32, hwc=False)
    assert rf.table.tolist() == [[[0, 20, 36, 17, 32], [2160, 20, 36, 17, 32]], [[4320, 40, 24, 32, 19], [7200, 40, 24, 32, 19]]]
    assert rf.flat.numel() == 2 * 3 * (20 * 36 + 40 * 24)


def test_prefetch_loader_passes_raw_frames_on_cpu():
    videos = _videos(shapes=[(2, 20, 36), (2, 40, 24)])
    ids = torch.arange(8).view(2, 4)
    raw_batches = [dict(visual_inputs=_raw(videos, size=32), text_input_ids=ids, n_examples_list=[1, 1], nested=[_raw(videos, size=32)[0:1]])
                   for _ in range(3)]
    got = list(data.PrefetchLoader(raw_batches, device="cpu"))
    assert len(got) == 3
    for b in got:
        rf = b["visual_inputs"]
        assert isinstance(rf, data.RawFrames) and rf.shape == (2, 2, 3, 32, 32) and rf.hwc and rf.max_img_size == 32
        assert torch.equal(_densify(rf), R.dense_batch(videos, 32)) and torch.equal(b["text_input_ids"], ids) and b["n_examples_list"] == [1, 1]
        assert isinstance(b["nested"][0], data.RawFrames) and torch.equal(_densify(b["nested"][0]), R.dense_batch(videos, 32)[0:1])
    plain = [dict(visual_inputs=torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), text_input_ids=ids, vid_id="v0", pair=(ids, [ids]))]
    (out,) = list(data.PrefetchLoader(plain, device="cpu"))                              # tensor-only batches: as before
    assert set(out) == set(plain[0]) and out["vid_id"] == "v0" and torch.equal(out["visual_inputs"], plain[0]["visual_inputs"])
    assert isinstance(out["pair"], tuple) and torch.equal(out["pair"][1][0], ids)


@pytest.mark.gpu
def test_prefetch_loader_stages_raw_frames_to_the_gpu():
    videos = _videos(shapes=[(2, 20, 36), (2, 40, 24)])
    other = _videos(seed=77, shapes=[(2, 24, 24), (2, 18, 30)])
    batches = [dict(visual_inputs=_raw(v, size=32), k=i) for i, v in enumerate([videos, other, videos, other])]
    for i, b in enumerate(data.PrefetchLoader(batches, device="cuda:0")):
        rf = b["visual_inputs"]
        assert rf.flat.is_cuda and rf.table.is_cuda and not rf.host_table.is_cuda and b["k"] == i
        assert torch.equal(rf.table.cpu(), rf.host_table)
        assert torch.equal(_densify(rf), R.dense_batch([videos, other][i % 2], 32))


# ---- 6. model level ---------------------------------------------------------------------------------------------------------------
def _inputs(cfg, hwc=True):
    videos = _videos()
    rf = _raw(videos, hwc)
    dense = R.image_norm(R.dense_batch(videos, SIZE), S.PIXEL_MEAN, S.PIXEL_STD)        # what the reference's loader hands to its model
    ids, mask = S.synthetic_text(4, 6, 5, cfg["vocab_size"])
    return rf, dense, ids.clamp(max=cfg["vocab_size"] - 1), mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hwc", [True, False])
def test_model_on_raw_frames_equals_model_on_resized_tensor(hw, dtype, hwc):
    cfg, sd, model = build("retrieval", RET, dtype, hw.dev)
    rf, dense, ids, mask = _inputs(cfg, hwc)
    common = dict(text_input_ids=ids, text_input_mask=mask, labels=torch.tensor([1, 0, 1, 0]))
    with torch.no_grad():
        a = model(dict(to_dev(common, hw.dev), visual_inputs=rf.to(hw.dev), n_examples_list=[2, 2]))
        b = model(dict(to_dev(common, hw.dev), visual_inputs=hw(dense), n_examples_list=[2, 2]))
        ga, gb = model.grid_features(rf.to(hw.dev)), model.grid_features(hw(dense))
    assert ga.shape == gb.shape
    err = (a["logits"].float() - b["logits"].float()).abs().max().item()
    print(f"RawFrames vs resized tensor, {dtype}: max |logit difference| {err:.3e} (bound {LOGIT_BOUND[dtype]:.0e})")
    assert err <= LOGIT_BOUND[dtype], err
    assert (a["loss"].float() - b["loss"].float()).abs().max().item() <= LOGIT_BOUND[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("fold", [True, False])
def test_clip_loop_on_raw_frames(hw, dtype, fold):
    cfg, sd, model = build("retrieval", RET, dtype, hw.dev)
    rf, dense, ids, mask = _inputs(cfg)
    common = to_dev(dict(text_input_ids=ids, text_input_mask=mask), hw.dev)
    with torch.no_grad():
        a = tasks.forward_clips_stack(model, dict(common, visual_inputs=rf.to(hw.dev), n_examples_list=[2, 2]), 2, 2, fold=fold)
        b = tasks.forward_clips_stack(model, dict(common, visual_inputs=hw(dense), n_examples_list=[2, 2]), 2, 2, fold=fold)
    assert a.shape == b.shape == (2, 4, 2)
    err = (a.float() - b.float()).abs().max().item()
    assert err <= LOGIT_BOUND[dtype], err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_step_on_raw_frames(hw, dtype):
    cfg, sd, model = build("retrieval", RET, dtype, hw.dev)
    model.train()
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
    tcfg = SimpleNamespace(train_n_clips=2, num_frm=2, score_agg_func="mean", learning_rate=1e-3, cnn_learning_rate=1e-3, decay="linear",
                           cnn_lr_decay="linear", num_train_steps=10, warmup_ratio=0.1, transformer_lr_mul=1.0, cnn_lr_mul=1.0)
    rf, _dense, ids, mask = _inputs(cfg)
    batch = dict(to_dev(dict(text_input_ids=ids, text_input_mask=mask, labels=torch.tensor([1, 0, 1, 0])), hw.dev),
                 visual_inputs=rf.to(hw.dev), n_examples_list=[2, 2])
    watched = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters()
               if n.endswith("pooler.dense.weight") or n.endswith("res5.2.conv3.weight")}
    assert len(watched) == 2
    loss = tasks.train_step(model, opt, batch, tcfg, global_step=0)
    assert torch.isfinite(loss).all()
    for n, p in model.named_parameters():
        if n in watched:
            assert not torch.equal(p.detach().float().cpu(), watched[n]), n           # the encoder AND the CNN were updated


@pytest.mark.gpu
def test_raw_frames_forward_is_graph_capturable():
    """The captured training step's constraint on the new op: no host synchronisation, geometry read on the device.  The CNN forward on
    a RawFrames is captured once into a hipGraph; new frames with ANOTHER geometry (same byte count) are then written into the captured
    buffer and table in place, and the replay must give what an eager forward gives on them."""
    dev = torch.device("cuda", 0)
    cfg, sd, model = build("retrieval", RET, torch.bfloat16, dev)
    first = _raw(_videos(seed=21, shapes=[(4, 48, 80), (4, 90, 60)])).to(dev)
    second = _raw(_videos(seed=31, shapes=[(4, 90, 60), (4, 48, 80)]))
    assert second.flat.numel() == first.flat.numel() and not torch.equal(second.table, first.host_table)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.no_grad(), torch.cuda.stream(side):
        eager_first = model.grid_features(first).float().clone()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = model.grid_features(first)
    first.flat.copy_(second.flat.to(dev))
    first.table.copy_(second.table.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.float().clone()
    with torch.no_grad():
        eager_second = model.grid_features(second.to(dev)).float()
    tol = 1e-2 * eager_second.abs().max().item()
    assert (replayed - eager_second).abs().max().item() <= tol
    assert (replayed - eager_first).abs().max().item() > tol                       # ... and not the frames it was captured with
