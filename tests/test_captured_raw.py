"""captured.CapturedStep(raw_frames=True): data.RawFrames batches replayed from captured step graphs.

The captured body reads an indirect RawFrames -- a static table buffer and one cb_frame_source descriptor -- so one graph serves every
native resolution and byte count; the pixel bytes stay where the batch put them.  GPU part: replays against the eager tasks.train_step
from the same state, step by step, held to the bounds of tests/test_captured_loop.py (its helpers are imported, not restated).  CPU part
(host emulator, ``mode="dry"``): the same run without graphs -- the whole indirect path --, the signature's ingredients, the eager
reasons that remain, and start_training(capture="dry") with cfg.capture_raw_frames."""
import warnings
from types import SimpleNamespace

import pytest
import torch

from clipbert_amd import captured as CAP
from clipbert_amd import data as D
from clipbert_amd import ops, optim, tasks
from test_captured_loop import (RET, _assert_same_step, _both, _snapshot, _tcfg, _text_batch, build_small, small_cpu, small_gpu)  # noqa: F401

S = 64
MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def _rgb_videos(i, hwc=True, videos=2, frames=2):
    """batch i: widths 56, heights 40 + 8 v + 4 i -- other native sizes and another byte count for every i"""
    g = torch.Generator().manual_seed(700 + i)
    shape = (lambda h: (frames, h, 56, 3)) if hwc else (lambda h: (frames, 3, h, 56))
    return [torch.randint(0, 256, shape(40 + 8 * v + 4 * i), dtype=torch.uint8, generator=g) for v in range(videos)]


def _yuv_videos(i, videos=2, frames=2):
    g = torch.Generator().manual_seed(800 + i)
    return [(torch.randint(0, 256, (frames, D.yuv420_frame_bytes(40 + 8 * v + 4 * i, 56)), dtype=torch.uint8, generator=g), 40 + 8 * v + 4 * i, 56)
            for v in range(videos)]


def _raw_batch(s, i, rf, per_video=2, txt_len=6):
    """_text_batch around the RawFrames, with token ids that do not repeat inside the batch: the word-embedding gradient is then one
    add per element, whatever order the workgroups retire in -- on the emulator, which runs workgroups on host threads, two EAGER steps
    from one state otherwise differ in that tensor by more than the bounds of _assert_same_step (drawn for the GPU) allow"""
    b = _text_batch(rf, per_video, txt_len, 60 + i, s.cfg["vocab_size"], s.dev)
    ids = b["text_input_ids"]
    unique = 1 + torch.randperm(s.cfg["vocab_size"] - 1, generator=torch.Generator().manual_seed(60 + i))[:ids.numel()]
    return dict(b, text_input_ids=unique.view(ids.shape).to(ids.dtype).to(s.dev), visual_inputs=rf.to(s.dev))


def _rgb_batches(s, n):
    return [_raw_batch(s, i, D.collate_raw_frames(_rgb_videos(i), S)) for i in range(n)]


def _run(s, stepper, tcfg, batches, first_step=0):
    for k, b in enumerate(batches, first_step):
        got, want = _both(s.model, s.opt, lambda: stepper.step(b, k), lambda: tasks.train_step(s.model, s.opt, b, tcfg, k))
        _assert_same_step(s.model, got, want, f"step {k}")


def _no_eager_warning(caught):
    assert not [str(w.message) for w in caught if "runs eagerly" in str(w.message)], [str(w.message) for w in caught]


def _check_replayed_rgb(s, mode):
    tcfg = _tcfg()
    batches = _rgb_batches(s, 4)
    assert len({b["visual_inputs"].flat.numel() for b in batches}) == 4
    stepper = CAP.CapturedStep(s.model, s.opt, tcfg, raw_frames=True, mode=mode)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _run(s, stepper, tcfg, batches)
    _no_eager_warning(caught)
    assert stepper.log == ["eager", "eager", "replay", "replay"], stepper.log
    assert stepper.stats["captures"] == 1 and stepper.stats["fallbacks"] == 0 and len(stepper.graphs) == 1, stepper.stats
    entry = next(iter(stepper.graphs.values()))
    last = batches[-1]["visual_inputs"]
    static = entry.static["visual_inputs"]
    # what a step adds to the staged traffic: the table; the bytes are named, not copied, and held until the next batch is staged
    assert static.flat is None and static.source is entry.source.desc and entry.source.flat is last.flat
    assert entry.bufs[CAP.CapturedStep.RAW_TABLE].shape == (4, 5) and torch.equal(static.table.cpu(), last.table.cpu())
    assert entry.source.desc.cpu().tolist() == [last.flat.data_ptr(), last.flat.numel()]
    assert not any(torch.is_tensor(v) and v.dtype == torch.uint8 and v.numel() > 16 for v in entry.bufs.values())
    return stepper


# ================================================================================================================================
# GPU
# ================================================================================================================================
@pytest.mark.gpu
def test_rgb_replays_equal_eager_steps(small_gpu):
    _check_replayed_rgb(small_gpu["retrieval"], "graph")


@pytest.mark.gpu
def test_yuv_layouts_are_two_signatures_captured_once_each(small_gpu):
    s = small_gpu["retrieval"]
    tcfg = _tcfg()
    stepper = CAP.CapturedStep(s.model, s.opt, tcfg, raw_frames=True)
    batches = [_raw_batch(s, i, D.collate_yuv_frames(_yuv_videos(i), S, layout=layout, matrix="bt709")) for layout in ("i420", "nv12") for i in range(3)]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        _run(s, stepper, tcfg, batches)
    _no_eager_warning(caught)
    assert stepper.log == ["eager", "eager", "replay"] * 2, stepper.log
    assert stepper.stats["captures"] == 2 and stepper.stats["fallbacks"] == 0 and len(stepper.graphs) == 2, stepper.stats


def _bad_copy(rf):
    """the same batch with a host (and device) table whose last row leaves the buffer"""
    host = rf.host_table.clone()
    host[-1, -1, 0] = rf.flat.numel() - 10
    return D.RawFrames(rf.flat, host.to(rf.table.device), rf.max_img_size, rf.hwc, host, rf.pixfmt, rf.matrix)


def _check_bad_row(s, mode):
    tcfg = _tcfg()
    good = _rgb_batches(s, 3)
    stepper = CAP.CapturedStep(s.model, s.opt, tcfg, raw_frames=True, mode=mode)
    for k in range(2):
        stepper.step(good[k], k)
    bad = dict(good[2], visual_inputs=_bad_copy(good[2]["visual_inputs"]))
    entry = next(iter(stepper.graphs.values()))
    before = _snapshot(s.model, s.opt)
    staged = {k: v.clone() for k, v in entry.bufs.items()}
    with pytest.raises(RuntimeError, match="cb_resize_pack_u8: frame 3 .*leaves the"):
        stepper.step(bad, 2)
    after = _snapshot(s.model, s.opt)
    assert after["step"] == before["step"] and after["fwd"] == before["fwd"]
    assert all(torch.equal(after[k], before[k]) for k in ("master", "m", "v", "seed"))
    assert all(torch.equal(v, entry.bufs[k]) for k, v in staged.items()) and entry.source.flat is good[1]["visual_inputs"].flat      # nothing was staged
    assert stepper.log == ["eager", "eager"] and stepper.stats["replays"] == 0
    got, want = _both(s.model, s.opt, lambda: stepper.step(good[2], 2), lambda: tasks.train_step(s.model, s.opt, good[2], tcfg, 2))
    _assert_same_step(s.model, got, want, "the good batch after the bad one")
    assert stepper.log == ["eager", "eager", "replay"]


@pytest.mark.gpu
def test_a_bad_row_raises_before_anything_runs(small_gpu):
    _check_bad_row(small_gpu["retrieval"], "graph")


# ================================================================================================================================
# host emulator: mode="dry"
# ================================================================================================================================
def test_dry_rgb_replays_equal_eager_steps(small_cpu):
    _check_replayed_rgb(small_cpu, "dry")


def _record_steps(monkeypatch):
    """bookkeeping only: the eager step is replaced by a recorder of the batch it was handed (as tests/test_captured_loop.py does)"""
    handed = []
    monkeypatch.setattr(tasks, "train_step", lambda model, opt, batch, *a, **kw: handed.append(batch) or torch.zeros(()))
    return handed


def test_dry_bad_row_raises_what_the_direct_launch_raises(small_cpu, monkeypatch):
    s = small_cpu
    handed = _record_steps(monkeypatch)
    good = _rgb_batches(s, 3)
    stepper = CAP.CapturedStep(s.model, s.opt, _tcfg(), raw_frames=True, mode="dry")
    for k in range(2):
        stepper.step(good[k], k)
    entry = next(iter(stepper.graphs.values()))
    staged = {k: v.clone() for k, v in entry.bufs.items()}
    bad = _bad_copy(good[2]["visual_inputs"])
    with pytest.raises(RuntimeError) as err:
        stepper.step(dict(good[2], visual_inputs=bad), 2)
    assert len(handed) == 2 and stepper.log == ["eager"] * 2                                  # neither staged nor stepped
    assert all(torch.equal(v, entry.bufs[k]) for k, v in staged.items()) and entry.source.flat is good[1]["visual_inputs"].flat
    table, host = bad.packed_table()
    with pytest.raises(RuntimeError) as direct:                                               # what the eager step's launch says of this batch
        ops.resize_pack_u8(bad.flat, table, 4, S, torch.float32, MEAN, STD, host_table=host)
    assert str(err.value) == str(direct.value) and "frame 3" in str(err.value) and "leaves the" in str(err.value)
    stepper.step(good[2], 2)
    assert stepper.log == ["eager", "eager", "replay"] and handed[-1] is entry.static and entry.source.flat is good[2]["visual_inputs"].flat


def test_eager_reasons_that_remain(small_cpu, monkeypatch):
    s = small_cpu
    rf = D.collate_raw_frames(_rgb_videos(0), S)
    b = _raw_batch(s, 0, rf)
    mk = lambda **kw: CAP.CapturedStep(s.model, s.opt, _tcfg(), mode="dry", **kw)      # noqa: E731
    assert mk(raw_frames=True)._why_eager(b) is None
    assert mk()._why_eager(b) == mk(raw_frames=False)._why_eager(b) == "RawFrames batch (launch geometry from its host table)"
    no_host = D.RawFrames(rf.flat, rf.table, S)
    no_host.host_table = None
    moved = rf.to("meta")
    indirect = D.RawFrames.indirect(D.FrameSource("cpu").desc, rf.table, S)
    handed = _record_steps(monkeypatch)
    for vis, reason in ((no_host, "without a host table"), (moved, "visual_inputs.flat is on meta, the model on cpu"), (indirect, "indirect already")):
        nb = dict(b, visual_inputs=vis)
        stepper = mk(raw_frames=True)
        why = stepper._why_eager(nb)
        assert why is not None and reason in why and "launch geometry" not in why, why
        # ... and such a batch runs the eager step on the batch itself, with one warning that names its reason
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            for k in range(3):
                stepper.step(nb, k)
                assert handed[-1] is nb
        mine = [str(w.message) for w in caught if "runs eagerly" in str(w.message)]
        assert len(mine) == 1 and reason in mine[0], mine
        assert stepper.log == ["eager"] * 3 and stepper.stats["fallbacks"] == 3 and not stepper.graphs


def test_signature_ignores_native_sizes_and_follows_what_fixes_the_launches(small_cpu):
    s = small_cpu
    stepper = CAP.CapturedStep(s.model, s.opt, _tcfg(), mode="dry", raw_frames=True)
    sig = lambda rf: stepper.signature(_raw_batch(s, 0, rf))                            # noqa: E731
    base = sig(D.collate_raw_frames(_rgb_videos(0), S))
    other_sizes = D.collate_raw_frames(_rgb_videos(3), S)
    assert other_sizes.flat.numel() != D.collate_raw_frames(_rgb_videos(0), S).flat.numel()
    assert sig(other_sizes) == base and hash(base) is not None                          # native sizes, byte count, table values: not in it
    i420, nv12 = (D.collate_yuv_frames(_yuv_videos(0), S, layout=l) for l in ("i420", "nv12"))
    other = [sig(i420), sig(nv12),                                                      # pixfmt
             sig(D.collate_yuv_frames(_yuv_videos(0), S, layout="i420", matrix="bt709")),                    # matrix
             sig(D.collate_raw_frames(_rgb_videos(0, hwc=False), S, hwc=False)),                             # hwc
             sig(D.collate_raw_frames(_rgb_videos(0), 48)),                                                  # max_img_size
             sig(D.collate_raw_frames(_rgb_videos(0, frames=4), S)),                                         # the leading shape
             stepper.signature(dict(_raw_batch(s, 0, other_sizes), visual_inputs=other_sizes.to("meta")))]   # device
    assert all(o != base for o in other) and len(set(other)) == len(other)
    assert sig(D.collate_yuv_frames(_yuv_videos(2), S, layout="nv12")) == sig(nv12)


class _Spy(CAP.CapturedStep):
    built = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        _Spy.built.append(self)


def test_start_training_reads_capture_raw_frames(small_cpu, monkeypatch):
    s = small_cpu
    _record_steps(monkeypatch)
    monkeypatch.setattr(CAP, "CapturedStep", _Spy)
    monkeypatch.setattr(_Spy, "built", [])
    loader = [_raw_batch(s, 0, D.collate_raw_frames(_rgb_videos(0), S))]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for kw in (dict(), dict(capture_raw_frames=0), dict(capture_raw_frames=1)):
            assert tasks.start_training(s.model, s.opt, loader, _tcfg(num_train_steps=3, **kw), capture="dry") == 3
        mine = CAP.CapturedStep(s.model, s.opt, _tcfg(), mode="dry", raw_frames=True)
        tasks.start_training(s.model, s.opt, loader, _tcfg(num_train_steps=3), capture=mine)     # a caller-built one is used as it is
    built = _Spy.built
    assert [b.raw_frames for b in built] == [False, False, True, True] and built[3] is mine
    assert [b.log for b in built] == [["eager"] * 3] * 2 + [["eager", "eager", "replay"]] * 2
    assert [b.stats["fallbacks"] for b in built] == [3, 3, 0, 0]                                 # default off: today's fallback
    from clipbert_amd import config
    assert config.SHARED_DEFAULTS["capture_raw_frames"] == 0


def test_start_training_with_capture_raw_frames_reaches_the_same_parameters(emul, monkeypatch):
    """six optimizer steps over six RawFrames batches (one frame and one caption each: the emulator runs every launch): capture="dry"
    with cfg.capture_raw_frames = 1 against the eager loop"""
    monkeypatch.setattr(CAP, "CapturedStep", _Spy)
    monkeypatch.setattr(_Spy, "built", [])
    dev = torch.device("cpu")
    finals = []
    for capture in (False, "dry"):
        cfg, _sd, model = build_small("retrieval", RET, torch.float32, dev)
        opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
        tcfg = _tcfg(train_n_clips=1, num_train_steps=6, warmup_ratio=0.5, train_batch_size=1, valid_steps=0, capture_raw_frames=1)
        s = SimpleNamespace(cfg=cfg, dev=dev)
        loader = [_raw_batch(s, i, D.collate_raw_frames(_rgb_videos(i, videos=1, frames=1), S), per_video=1, txt_len=4) for i in range(6)]
        assert tasks.start_training(model, opt, loader, tcfg, capture=capture) == 6 and opt.step_count == 6
        finals.append(model.rt.bank.master.clone())
    (stepper,) = _Spy.built
    assert stepper.raw_frames and stepper.log == ["eager"] * 2 + ["replay"] * 4, stepper.log
    assert stepper.stats["captures"] == 1 and stepper.stats["fallbacks"] == 0, stepper.stats
    assert float((finals[0] - finals[1]).abs().max()) <= 1e-6 * float(finals[0].abs().max())
