"""The retrieval evaluation on the device -- tasks.inference_retrieval_matrix / eval_retrieval_matrix / retrieval_rows /
gather_retrieval_matrix -- against the existing host path (tasks.inference_retrieval / eval_retrieval, left as they are) on the small
model, with == equality throughout: both paths run the same encoder passes, the same pooling and the same cb_retrieval_scores launches,
so the fp32 scores are the same bits, and the integer keys are exactly the rounded scores.

5 videos x 7 captions: both counts are at most 16, the length up to which torch's unstable descending sort (the existing path's, and the
reference's) coincides with the stable order the device path defines -- the synthetic model barely separates the captions, so after
rounding to 4 places the matrix is full of ties, and the metrics of the two paths are still equal."""
import functools
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import retrieval_rank_restatement as R
from clipbert_amd import ops, tasks
from clipbert_amd import synthetic as S
from oracle import clipbert_oracle as O
from test_model_small import build, to_dev

N_VIDEOS, N_CAPTIONS, EVAL_BSZ = 5, 7, 3
TXT_IDS = [f"cap{j}" for j in range(N_CAPTIONS)]
GT = {t: f"video{(2 * j + 1) % N_VIDEOS}" for j, t in enumerate(TXT_IDS)}      # every video owns a caption, two of them own two


def _content_key(x):
    if torch.is_tensor(x):
        return (str(x.dtype), tuple(x.shape), hashlib.sha1(x.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest())
    if isinstance(x, dict):
        return tuple((k, _content_key(v)) for k, v in sorted(x.items()))
    return repr(x)


def _memoise(model, name):
    """every model pass costs the host emulator about a second, and the cases below repeat the same passes (the two loops under comparison,
    the three pooling methods, the merge and validation tests): on the emulator a pass with the SAME input bytes is computed once per
    process and its output handed out as a fresh copy.  Everything downstream of the passes -- the pooling, cb_retrieval_scores, where a
    score lands -- still runs every time; on the GPU nothing is memoised."""
    fn, cache = getattr(model, name), {}

    def wrapper(arg):
        key = (model.training, _content_key(arg))
        if key not in cache:
            cache[key] = fn(arg)
        out = cache[key]
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in out.items()} if isinstance(out, dict) else out.clone()

    setattr(model, name, wrapper)


@functools.lru_cache(maxsize=None)
def _small(c, dtype, dev):
    """(cfg, model in eval mode) per (num_labels, dtype, device): built once, only ever run forward"""
    cfg, _sd, model = build("retrieval", dict(num_labels=c, loss_type="ce", margin=0.1), dtype, torch.device(dev))
    model.eval()
    if torch.device(dev).type == "cpu":
        for name in ("grid_features", "forward_from_grid", "forward"):
            _memoise(model, name)
    return cfg, model


def _videos(cfg, n_clips, dev, n_videos=N_VIDEOS, seed=31):
    """one dict per video, as the retrieval evaluation set yields them: (1, n_clips, 3, 64, 64) frames (num_frm = 1) against the same 7
    captions"""
    frames = O.image_norm(S.synthetic_frames(n_videos, n_clips, 64, seed), S.PIXEL_MEAN, S.PIXEL_STD)
    ids, mask = S.synthetic_text(N_CAPTIONS, 6, seed, cfg["vocab_size"])
    ids = ids.clamp(max=cfg["vocab_size"] - 1)
    return [to_dev(dict(vid_id=f"video{i}", visual_inputs=frames[i:i + 1].contiguous(), text_input_ids=ids, text_input_mask=mask,
                        caption_ids=list(TXT_IDS)), dev) for i in range(n_videos)]


def _icfg(n_clips, pool):
    return SimpleNamespace(inference_n_clips=n_clips, num_frm=1, score_agg_func=pool, inference_batch_size=EVAL_BSZ)


def _keys_of_rows(rows, vid_ids, txt_ids):
    """rint(1e4 * score) of the existing path's dict rows as a (videos, captions) integer matrix"""
    at = {(r["vid_id"], r["txt_id"]): r["score"] for r in rows}
    assert len(at) == len(rows) == len(vid_ids) * len(txt_ids)
    return np.array([[int(np.rint(1e4 * at[v, t])) for t in txt_ids] for v in vid_ids], dtype=np.int64)


def _assert_equals_the_host_path(matrix, rows, metrics):
    assert matrix.vid_ids == [f"video{i}" for i in range(N_VIDEOS)] and matrix.txt_ids == TXT_IDS
    assert matrix.scores.dtype == torch.float32 and tuple(matrix.scores.shape) == (N_VIDEOS, N_CAPTIONS)
    scores = matrix.scores.cpu().numpy()
    want_keys = _keys_of_rows(rows, matrix.vid_ids, matrix.txt_ids)
    assert np.array_equal(R.keys(scores), want_keys)
    assert [round(float(p), 4) for p in scores.reshape(-1)] == [r["score"] for r in rows]      # (the rows are video-major too)
    assert tasks.retrieval_rows(matrix) == rows
    got = tasks.eval_retrieval_matrix(matrix, GT)
    assert got == metrics == tasks.eval_retrieval(rows, GT)
    vid_idx, txt_idx = {v: i for i, v in enumerate(matrix.vid_ids)}, {t: j for j, t in enumerate(TXT_IDS)}
    gt_v2t = {v: t for t, v in GT.items()}
    for kind, axis, gt in (("text2video", R.COL_QUERIES, [vid_idx[GT[t]] for t in TXT_IDS]),
                           ("video2text", R.ROW_QUERIES, [txt_idx[gt_v2t[v]] for v in matrix.vid_ids])):
        want = R.ranks_by_counting(scores, gt, axis)
        dev_gt = torch.tensor(gt, dtype=torch.int32).to(matrix.scores.device)
        assert np.array_equal(ops.retrieval_rank(matrix.scores, dev_gt, axis).cpu().numpy(), want)
        assert got[kind] == tasks.retrieval_metrics_from_ranks(want)
    n_ties = scores.size - len(np.unique(want_keys))
    print(f"{n_ties} of {scores.size} rounded scores repeat another one; text2video {got['text2video']}")


@pytest.mark.parametrize("pool", ["mean", "max", "lse"])
@pytest.mark.parametrize("n_clips", [1, 3])
@pytest.mark.parametrize("c", [2, 1])
def test_matrix_path_equals_the_host_path(hw, c, n_clips, pool):
    """the existing loop run eagerly against the matrix loop with capture="dry" (the CapturedForward bookkeeping, graphs or not): 3 text
    mini-batches per video (3 + 3 + 1 captions), one encoder pass over all clips each"""
    cfg, model = _small(c, torch.float32, str(hw.dev))
    videos, icfg = _videos(cfg, n_clips, hw.dev), _icfg(n_clips, pool)
    try:
        rows, metrics = tasks.inference_retrieval(model, videos, icfg, GT)
        matrix = tasks.inference_retrieval_matrix(model, videos, icfg, capture="dry")
        assert model._captured_forward.mode == "dry" and model._captured_forward.stats["failed_captures"] == 0
    finally:
        model._captured_forward = None
    assert matrix.scores.device == videos[0]["text_input_ids"].device
    _assert_equals_the_host_path(matrix, rows, metrics)


def test_per_clip_order_of_evaluation(hw):
    """cache_cnn=False (the reference's order of evaluation: a full forward per clip per mini-batch) on the first three videos, one clip
    each: the matrix loop gives the existing loop's rows with the same switch, and the matrix of cache_cnn=True -- with one clip both
    orders run the CNN and the encoder on batches of the same shapes, so the fp32 scores are the same bits"""
    cfg, model = _small(2, torch.float32, str(hw.dev))
    videos, icfg = _videos(cfg, 1, hw.dev)[:3], _icfg(1, "lse")
    gt = {t: f"video{j % 3}" for j, t in enumerate(TXT_IDS)}
    rows, metrics = tasks.inference_retrieval(model, videos, icfg, gt, cache_cnn=False)
    matrix = tasks.inference_retrieval_matrix(model, videos, icfg, cache_cnn=False)
    assert matrix.vid_ids == ["video0", "video1", "video2"] and tasks.retrieval_rows(matrix) == rows
    assert tasks.eval_retrieval_matrix(matrix, gt) == metrics
    cached = tasks.inference_retrieval_matrix(model, videos, icfg, cache_cnn=True)
    assert cached.vid_ids == matrix.vid_ids and cached.txt_ids == matrix.txt_ids and torch.equal(cached.scores, matrix.scores)
    with pytest.raises(ValueError, match="cache_cnn=True only"):
        tasks.inference_retrieval_matrix(model, videos, icfg, cache_cnn=False, capture="dry")


@pytest.mark.gpu
def test_graph_replays_equal_eager():
    """bf16 model, hipGraph replays of the encoder passes (two signatures: 3 and 1 captions x 3 clips): the matrix is the eager matrix, bit
    for bit, and equals the host path run from the same graphs"""
    dev = torch.device("cuda", 0)
    cfg, model = _small(2, torch.bfloat16, str(dev))
    videos, icfg = _videos(cfg, 3, dev), _icfg(3, "lse")
    eager = tasks.inference_retrieval_matrix(model, videos, icfg)
    try:
        captured = tasks.inference_retrieval_matrix(model, videos, icfg, capture=True)
        cf = model._captured_forward
        assert cf.mode == "graph" and cf.stats["captures"] == 2 and cf.stats["failed_captures"] == 0, cf.stats
        assert cf.log.count("replay") == len(cf.log) - 4, cf.log
        rows, metrics = tasks.inference_retrieval(model, videos, icfg, GT, capture=True)
    finally:
        model._captured_forward = None
    assert torch.equal(captured.scores, eager.scores)
    _assert_equals_the_host_path(captured, rows, metrics)


def test_matrix_handling(hw):
    """unequal caption lists raise and name the general path; a repeated video keeps its first row and is not evaluated again; an iterable
    without a length works; the pure merge of two ranks' parts is the single-process matrix"""
    cfg, model = _small(2, torch.float32, str(hw.dev))
    videos, icfg = _videos(cfg, 1, hw.dev), _icfg(1, "mean")
    whole = tasks.inference_retrieval_matrix(model, videos, icfg)
    other = dict(videos[1], caption_ids=TXT_IDS[:-1] + ["cap99"])
    with pytest.raises(ValueError, match="use inference_retrieval, the general path"):
        tasks.inference_retrieval_matrix(model, [videos[0], other], icfg)
    with pytest.raises(ValueError, match="no videos"):
        tasks.inference_retrieval_matrix(model, [], icfg)
    # video1 again, with video3's frames under its name: the first occurrence stays
    again = dict(videos[3], vid_id="video1")
    dup = tasks.inference_retrieval_matrix(model, (v for v in videos[:3] + [again] + videos[3:]), icfg)
    assert dup.vid_ids == whole.vid_ids and torch.equal(dup.scores, whole.scores)
    # two "ranks": the strided shards of shard_for_rank, rank 1 holding a copy of rank 0's first video on top
    parts = []
    for rank in range(2):
        mine = [videos[i] for i in tasks.shard_for_rank(N_VIDEOS, rank, 2)] + ([again, videos[0]] if rank == 1 else [])
        local = tasks.inference_retrieval_matrix(model, mine, icfg)
        assert tasks.gather_retrieval_matrix(local) is local                        # no process group: unchanged
        parts.append((local.vid_ids, local.txt_ids, local.scores.cpu().numpy()))
    before = [p[2].copy() for p in parts]
    vid_ids, txt_ids, block = tasks.merge_retrieval_parts(parts)
    assert all(np.array_equal(p[2], b) for p, b in zip(parts, before))
    assert vid_ids == ["video0", "video2", "video4", "video1", "video3"] and txt_ids == TXT_IDS and block.dtype == np.float32
    order = [int(v[5:]) for v in vid_ids]
    assert np.array_equal(block, whole.scores.cpu().numpy()[order])
    merged = tasks.RetrievalMatrix(vid_ids, txt_ids, hw(torch.from_numpy(block)))
    assert tasks.eval_retrieval_matrix(merged, GT) == tasks.eval_retrieval(tasks.retrieval_rows(merged), GT)
    by_pair = {(r["vid_id"], r["txt_id"]): r["score"] for r in tasks.retrieval_rows(whole)}
    assert {(r["vid_id"], r["txt_id"]): r["score"] for r in tasks.retrieval_rows(merged)} == by_pair
    with pytest.raises(ValueError, match="other captions than rank 0"):
        tasks.merge_retrieval_parts([parts[0], (parts[1][0], TXT_IDS[::-1], parts[1][2])])


def test_validate_retrieval_on_device(hw):
    """the log dict of validate_retrieval(on_device=True) is the default's"""
    cfg, model = _small(2, torch.float32, str(hw.dev))
    videos, icfg = _videos(cfg, 1, hw.dev, n_videos=N_VIDEOS), _icfg(1, "mean")
    frames = O.image_norm(S.synthetic_frames(2, 1, 64, 77), S.PIXEL_MEAN, S.PIXEL_STD)
    ids, mask = S.synthetic_text(4, 6, 77, cfg["vocab_size"])
    val = [to_dev(dict(visual_inputs=frames, text_input_ids=ids.clamp(max=cfg["vocab_size"] - 1), text_input_mask=mask,
                       labels=torch.tensor([1, 0, 0, 1]), n_examples_list=[2, 2], caption_ids=["a", "b", "c", "d"], vid_id=["x", "y"]), hw.dev)]
    for was_training in (False, True):
        model.train(was_training)
        try:
            want = tasks.validate_retrieval(model, val, videos, icfg, GT)
            got = tasks.validate_retrieval(model, val, videos, icfg, GT, on_device=True)
            assert model.training is was_training
        finally:
            model.eval()
        assert got == want and set(got) == {"valid/loss", "valid/acc"} | {f"valid/{k}_{m}" for k in ("text2video", "video2text")
                                                                          for m in ("r1", "r5", "r10", "medianR", "meanR")}
    assert set(tasks.validate_retrieval(model, val, videos, icfg, None, on_device=True)) == {"valid/loss", "valid/acc"}
