"""GPU-side input pipeline: what sits between the reference's DataLoader and ``ClipBert.forward``.

Reference: src/datasets/dataloader.py:86-152 ``PrefetchLoader`` -- a side stream that ``.cuda()``s the next collated batch
while the current one computes, then ``.float()`` and ``ImageNorm`` on the GPU (a 4-byte-per-pixel fp32 tensor is
materialised per batch).  Here

* frames stay **uint8** all the way into HBM (1 byte per pixel over PCIe and in HBM); the cast, mean / std and the RGB->BGR
  flip happen inside the stem's input pack (``cb_stem_pack(src_u8=1)``) -- ``img_normalize`` is therefore not a tensor op here
  but the (mean, std) pair handed to the model;
* that holds for the decoder's **native-resolution** frames too: ``RawFrames`` (built by ``collate_raw_frames``) carries a
  ragged batch -- every video its own height and width -- as one flat uint8 buffer plus a geometry table, and the reference's
  per-frame ``ImageResize`` (bilinear, longer side -> max_img_size) + ``ImagePad`` (src/datasets/dataset_base.py:270-273,
  src/datasets/data_utils.py:112-253) run on the GPU inside ``cb_resize_pack_u8``, which writes the stem's packed image
  directly.  No fp32 frame is ever built on the host;
* ... and for the decoder's own **YUV 4:2:0 planes** (``collate_yuv_frames``: I420 from software decoders, NV12 from hardware
  ones): the same ``RawFrames`` with ``pixfmt`` / ``matrix`` set, 1.5 bytes per pixel instead of 3, no colour conversion in the
  loader workers -- ``cb_resize_pack_yuv420`` converts each bilinear tap in the same launch;
* host staging is **pinned and double-buffered**: two pinned slots per tensor key, batch i+1 is copied host->pinned->HBM on a
  side HIP stream while batch i computes; a slot is reused only after the event recorded behind its last H2D copy has
  completed, and the consumer stream waits on the copy's event (not on the whole side stream);
* ``InfiniteIterator`` as in the reference (:155-175).

Host code + HIP streams / events (through torch): plumbing, no arithmetic."""
from typing import Dict, Iterable, Iterator, Optional, Sequence

import torch


# ---- the reference's resize arithmetic (host integers only) ------------------------------------------------------------------
def resize_size(h: int, w: int, max_size: int):
    """(new_h, new_w) of the reference's ImageResize (get_resize_size, src/datasets/data_utils.py:167-199): the longer side becomes
    ``max_size``, the shorter one ``max_size * short / long`` evaluated in Python floats and TRUNCATED (333 x 500 at 768 ->
    511 x 768, not 512); a square frame counts as portrait.  Pinned to the reference by tests/test_resize_pack.py."""
    long_side, short_side = max(h, w), min(h, w)
    other = int(max_size * (short_side / long_side))
    return (int(max_size), other) if h >= w else (other, int(max_size))


def is_extreme_aspect_ratio(h: int, w: int, max_ratio: float = 5.) -> bool:
    """longer side / shorter side > max_ratio: the videos the reference's dataset skips before it resizes them
    (_is_extreme_aspect_ratio, src/datasets/dataset_base.py:224-232)"""
    return max(h, w) > max_ratio * min(h, w)


class RawFrames:
    """A ragged batch of native-resolution uint8 RGB frames standing for the (B, T, 3, S, S) tensor the reference's collate would
    have produced from them (S = ``max_img_size``): resized, zero-padded, not yet normalised.

    ``flat``: 1-D uint8, all frames back to back -- interleaved (h, w, 3) each when ``hwc`` (what the decoder hands over before
    its permute, src/datasets/dataset_base.py:136-146), planar (3, h, w) otherwise.  ``table``: int64 (*lead, 5), one row
    [byte_offset, h, w, new_h, new_w] per frame, on ``flat``'s device; ``host_table``: the same rows on the host (argument
    validation at launch time without a device read).  The leading dimensions ``lead`` are the batch dimensions of the tensor
    it stands for: ``view`` / ``reshape`` / ``transpose`` / indexing / ``contiguous`` act on them exactly as they would on that
    tensor, by permuting and slicing the TABLE ROWS only -- pixel bytes are never copied on the host, and frames a slice leaves
    out simply are not referenced any more -- and still travel: ``to`` / ``PrefetchLoader`` upload the WHOLE ``flat`` buffer of a
    sliced RawFrames (slice on the device, after the copy; re-collate on the host to ship less).  The model consumes it wherever it takes a frame tensor (modeling.cnn_forward).

    ``pixfmt``: "rgb" (the above) or "i420" / "nv12" -- every frame is then its tightly packed YUV 4:2:0 planes (Y h x w, then U and V
    of ceil(h / 2) x ceil(w / 2) each, or the two interleaved; ``hwc`` is ignored) and ``matrix`` ("bt601": limited range, what
    libswscale applies to an untagged stream; "bt601-full", "bt709", "bt709-full") is the conversion it stands for: the RGB frames
    tests/yuv_restatement.py spells out, nearest chroma, rounded to uint8 before the resize.

    ``source``: None, or the descriptor of the indirect form (``RawFrames.indirect``: ``flat`` is then None)."""
    PIXFMTS = ("rgb", "i420", "nv12")
    MATRICES = ("bt601", "bt601-full", "bt709", "bt709-full")

    def __init__(self, flat: Optional[torch.Tensor], table: torch.Tensor, max_img_size: int, hwc: bool = True,
                 host_table: Optional[torch.Tensor] = None, pixfmt: str = "rgb", matrix: str = "bt601", source: Optional[torch.Tensor] = None):
        if source is None:
            assert flat is not None and flat.dtype == torch.uint8 and flat.dim() == 1
        else:                                   # the indirect form (RawFrames.indirect)
            assert flat is None and tuple(source.shape) == ((16,) if source.dtype == torch.uint8 else (2,)) and \
                source.dtype in (torch.uint8, torch.int64) and source.is_contiguous() and source.device == table.device, "source: uint8 (16,) or int64 (2,) beside the table"
        assert table.dtype == torch.int64 and table.dim() >= 1 and table.shape[-1] == 5
        if host_table is None and not table.is_cuda and source is None:
            host_table = table
        assert host_table is None or (not host_table.is_cuda and host_table.shape == table.shape)
        self.flat, self.table, self.host_table, self.source = flat, table, host_table, source
        assert pixfmt in self.PIXFMTS and matrix in self.MATRICES, (pixfmt, matrix)
        self.max_img_size, self.hwc = int(max_img_size), bool(hwc)
        self.pixfmt, self.matrix = pixfmt, matrix

    @classmethod
    def indirect(cls, source: torch.Tensor, table: torch.Tensor, max_img_size: int, hwc: bool = True,
                 host_table: Optional[torch.Tensor] = None, pixfmt: str = "rgb", matrix: str = "bt601") -> "RawFrames":
        """The INDIRECT form: the pixels are named by a descriptor in device memory instead of ``flat`` (which is None) -- ``source``,
        uint8 (16,) or int64 (2,) on the table's device: a cb_frame_source {base address, byte count}, which the kernel reads at run
        time (cb_resize_pack_u8_src / cb_resize_pack_yuv420_src).  Whoever owns the descriptor re-points it between launches
        (``FrameSource``) and keeps the bytes alive; a descriptor of 0 bytes, and every row that leaves its byte count, is an
        all-padding frame.  It is what a captured step sees in place of the batch (captured.CapturedStep(raw_frames=True)): table and
        descriptor keep their addresses, their contents change per step.  Everything that acts on the table rows works as on the
        direct form; ``to`` raises (the address in the descriptor means nothing elsewhere).  No host table unless one is given: the
        launch validates none."""
        return cls(None, table, max_img_size, hwc, host_table, pixfmt, matrix, source=source)

    def _with(self, flat, table, host_table):
        """the same kind of frames (size, layout, pixel format, matrix) over other tensors"""
        return RawFrames(flat, table, self.max_img_size, self.hwc, host_table, self.pixfmt, self.matrix)

    def _like(self, table, host_table):
        if self.source is not None:
            return RawFrames.indirect(self.source, table, self.max_img_size, self.hwc, host_table, self.pixfmt, self.matrix)
        return self._with(self.flat, table, host_table)

    def _both(self, fn):
        """the same table-row operation on the device table and its host copy"""
        if self.host_table is None or self.host_table is self.table:
            t = fn(self.table)
            return self._like(t, t if self.host_table is not None else None)
        return self._like(fn(self.table), fn(self.host_table))

    # ---- what the task loops ask of batch["visual_inputs"] --------------------------------------------------------------------
    @property
    def shape(self) -> torch.Size:
        return torch.Size(tuple(self.table.shape[:-1]) + (3, self.max_img_size, self.max_img_size))

    @property
    def device(self):
        return self.table.device if self.flat is None else self.flat.device

    dtype = torch.uint8

    def dim(self) -> int:
        return self.table.dim() + 2

    def size(self, d: Optional[int] = None):
        return self.shape if d is None else self.shape[d]

    def __len__(self):
        return self.shape[0]

    @property
    def n_frames(self) -> int:
        return self.table.numel() // 5

    def _lead(self, shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        tail = (3, self.max_img_size, self.max_img_size)
        if len(shape) < 3 or tuple(int(d) for d in shape[-3:]) != tail:
            raise ValueError(f"RawFrames: only the leading (batch) dimensions can be regrouped; {tuple(shape)} must end in {tail}")
        return tuple(int(d) for d in shape[:-3])

    def view(self, *shape):
        lead = self._lead(shape)
        return self._both(lambda t: t.view(*lead, 5))

    def reshape(self, *shape):
        lead = self._lead(shape)
        return self._both(lambda t: t.reshape(*lead, 5))

    def transpose(self, d0: int, d1: int):
        nl = self.table.dim() - 1
        if not (0 <= d0 < nl and 0 <= d1 < nl):
            raise ValueError("RawFrames: only the leading (batch) dimensions can be transposed")
        return self._both(lambda t: t.transpose(d0, d1))

    def __getitem__(self, idx):
        idx = idx if isinstance(idx, tuple) else (idx,)
        if len(idx) > self.table.dim() - 1 or any(not isinstance(i, (int, slice)) for i in idx):
            raise IndexError("RawFrames: integer / slice indices over the leading (batch) dimensions only")
        return self._both(lambda t: t[idx])

    def is_contiguous(self) -> bool:
        return self.table.is_contiguous()

    def contiguous(self):
        return self if self.is_contiguous() else self._both(lambda t: t.contiguous())

    def to(self, device, non_blocking: bool = False):
        if self.source is not None:
            raise RuntimeError("RawFrames.to(): an indirect RawFrames names its bytes by a device address and cannot travel; move the direct one")
        device = torch.device(device)
        host = self.host_table if self.host_table is not None else (self.table if not self.table.is_cuda else None)
        return self._with(self.flat.to(device, non_blocking=non_blocking), self.table.to(device, non_blocking=non_blocking), host)

    def packed_table(self):
        """(table, host_table) as contiguous (n_frames, 5) row lists in the order of the leading dimensions (what the kernel reads)"""
        t = self.table.reshape(-1, 5).contiguous()
        if self.host_table is None:
            return t, None
        return t, (t if self.host_table is self.table else self.host_table.reshape(-1, 5).contiguous())

    def __repr__(self):
        kind = f"hwc={self.hwc}" if self.pixfmt == "rgb" else f"pixfmt={self.pixfmt}, matrix={self.matrix}"
        where = "indirect" if self.flat is None else f"bytes={self.flat.numel()}"
        return f"RawFrames(shape={tuple(self.shape)}, {where}, {kind}, device={self.device})"


class FrameSource:
    """The descriptor of an indirect RawFrames and its owner: ``desc``, int64 (2,) [base address, byte count] on ``device`` (a
    cb_frame_source; 0 bytes until first pointed at something), and ``point_at(flat)``, which re-points it on the current stream and
    holds ``flat`` until the next call.  On a GPU the two words travel through a pinned two-slot buffer, a slot being rewritten only
    after the event behind its last upload has completed -- FusedAdamW.prepare_step's scheme; like it, never inside a capture."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.desc = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.flat = None                               # what the descriptor names: kept alive here
        self._cuda = self.device.type == "cuda"
        self._host = torch.zeros(2, 2, dtype=torch.int64).pin_memory() if self._cuda else None
        self._events = [None, None]
        self._n = 0

    def point_at(self, flat: Optional[torch.Tensor]):
        """desc = {flat.data_ptr(), flat.numel()} ({0, 0} for None), ordered on the current stream of the device"""
        if flat is not None:
            assert flat.dtype == torch.uint8 and flat.dim() == 1 and flat.is_contiguous() and flat.device == self.device, "a flat uint8 buffer on the descriptor's device"
        words = (flat.data_ptr(), flat.numel()) if flat is not None and flat.numel() else (0, 0)
        if not self._cuda:
            self.desc[0], self.desc[1] = words
        else:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FrameSource.point_at() inside a hipGraph capture: a graph would freeze the address it is meant to replace")
            slot = self._n & 1
            self._n += 1
            ev = self._events[slot]
            if ev is not None:
                ev.synchronize()                       # the copy that last read this slot has executed
            host = self._host[slot]
            host[0], host[1] = words
            with torch.cuda.device(self.device):
                self.desc.copy_(host, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            self._events[slot] = ev
        self.flat = flat


def _frame_rows(rows, off: int, t: int, h: int, w: int, frame_bytes: int, max_img_size: int) -> int:
    """append the table rows of one video's ``t`` frames of h x w, ``frame_bytes`` each, starting at byte ``off`` -> the next offset"""
    nh, nw = resize_size(h, w, max_img_size)
    if min(h, w, nh, nw) < 1:
        raise ValueError(f"a {h} x {w} frame resizes to {nh} x {nw} at max_img_size {max_img_size} (is_extreme_aspect_ratio videos are skipped by the dataset)")
    for _ in range(t):
        rows.append([off, h, w, nh, nw])
        off += frame_bytes
    return off


def collate_raw_frames(videos: Sequence[torch.Tensor], max_img_size: int, hwc: bool = True) -> RawFrames:
    """The frame half of the reference's collate for frames that were NOT resized by the dataset: ``videos`` holds one uint8 tensor
    per video, (T, h, w, 3) when ``hwc`` (the decoder's layout) or (T, 3, h, w) otherwise, the same T everywhere, any h x w per
    video -> the RawFrames standing for the (B, T, 3, S, S) batch.  One concatenation of the bytes; nothing is resized here."""
    assert len(videos) > 0
    t0 = videos[0].shape[0]
    rows, chunks, off = [], [], 0
    for v in videos:
        assert v.dtype == torch.uint8 and v.dim() == 4 and v.shape[0] == t0, "every video contributes the same number of uint8 frames"
        assert v.shape[3 if hwc else 1] == 3, f"expected {'(T, h, w, 3)' if hwc else '(T, 3, h, w)'} frames, got {tuple(v.shape)}"
        h, w = (v.shape[1], v.shape[2]) if hwc else (v.shape[2], v.shape[3])
        off = _frame_rows(rows, off, t0, h, w, 3 * h * w, max_img_size)
        chunks.append(v.contiguous().view(-1))
    table = torch.tensor(rows, dtype=torch.int64).view(len(videos), t0, 5)
    return RawFrames(torch.cat(chunks), table, max_img_size, hwc)


def yuv420_frame_bytes(h: int, w: int) -> int:
    """bytes of one tightly packed YUV 4:2:0 frame (I420 and NV12 alike): the luma plane and two chroma planes of half the size, rounded up"""
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def collate_yuv_frames(videos: Sequence, max_img_size: int, layout: str = "i420", matrix: str = "bt601") -> RawFrames:
    """collate_raw_frames for the decoder's YUV 4:2:0 planes: ``videos`` holds one ``(frames_u8, h, w)`` per video, ``frames_u8`` a
    (T, yuv420_frame_bytes(h, w)) uint8 tensor whose rows are the frames' planes -- ``layout`` "i420": Y, U, V (for even sizes PyAV's
    ``frame.to_ndarray(format="yuv420p")`` flattened); "nv12": Y, then interleaved UV -- the same T everywhere, any h x w per video.
    ``matrix``: the conversion the stream asks for (RawFrames).  One concatenation of the bytes; nothing is converted or resized here."""
    assert len(videos) > 0 and layout in ("i420", "nv12") and matrix in RawFrames.MATRICES, (layout, matrix)
    t0 = videos[0][0].shape[0]
    rows, chunks, off = [], [], 0
    for v, h, w in videos:
        h, w = int(h), int(w)
        assert v.dtype == torch.uint8 and v.dim() == 2 and v.shape[0] == t0, "every video contributes the same number of uint8 frames"
        assert v.shape[1] == yuv420_frame_bytes(h, w), f"a {h} x {w} 4:2:0 frame has {yuv420_frame_bytes(h, w)} bytes, got {v.shape[1]}"
        off = _frame_rows(rows, off, t0, h, w, v.shape[1], max_img_size)
        chunks.append(v.contiguous().view(-1))
    table = torch.tensor(rows, dtype=torch.int64).view(len(videos), t0, 5)
    return RawFrames(torch.cat(chunks), table, max_img_size, pixfmt=layout, matrix=matrix)


# ---- VQA targets kept sparse (host lists -> two small tables) ----------------------------------------------------------------
def vqa_sparse_targets(answers: Sequence[Dict[str, float]], ans2label: Dict[str, int], max_answers: int = 10):
    """The soft targets of ``len(answers)`` questions -- each a dict answer -> score, as the annotations carry them -- as fixed-shape
    tables for cb_vqa_loss_fwd / _bwd: (ids int32 (n, K), scores fp32 (n, K)), K = max_answers, slots in the dict's order, padding id -1
    with score 0.  What ClipBertVQADataset._get_vqa_targets (src/datasets/dataset_vqa.py:57-72) scatters into num_labels zeros per
    question; an answer missing from ``ans2label`` raises KeyError as its line 68 does, more than ``max_answers`` answers ValueError."""
    n, k = len(answers), int(max_answers)
    ids = torch.full((n, k), -1, dtype=torch.int32)
    scores = torch.zeros((n, k), dtype=torch.float32)
    for i, ans2score in enumerate(answers):
        if len(ans2score) > k:
            raise ValueError(f"question {i} has {len(ans2score)} answers, the tables hold max_answers = {k}")
        for j, (ans, score) in enumerate(ans2score.items()):
            ids[i, j] = ans2label[ans]
            scores[i, j] = score
    return ids, scores


def vqa_dense_targets(ids: torch.Tensor, scores: torch.Tensor, num_labels: int) -> torch.Tensor:
    """the inverse of vqa_sparse_targets: fp32 (n, num_labels) targets, the scatter of _get_vqa_targets (padding slots -- id < 0 or
    >= num_labels -- dropped); the reference's batch format, for the dense ``labels`` path and the tests"""
    ids, scores = ids.cpu().long(), scores.cpu().float()
    valid = (ids >= 0) & (ids < num_labels)
    dense = torch.zeros(ids.shape[0], num_labels + 1, dtype=torch.float32)
    dense.scatter_(1, torch.where(valid, ids, torch.full_like(ids, num_labels)), torch.where(valid, scores, torch.zeros_like(scores)))
    return dense[:, :num_labels].contiguous()


# ---- masked-LM slots for device-drawn masks -----------------------------------------------------------------------------------------
def mlm_capacity(rows: int, p: float = 0.15, sigmas: float = 6.0) -> int:
    """The slot count for cfg.mlm_capacity when the labels are drawn per step (cfg.mlm_masking = "device"): a captured step needs a fixed
    capacity, and the count of labelled rows among ``rows`` text rows (B * Lt; special and pad rows only lower it) is binomial --
    min(rows, ceil(rows p + sigmas sqrt(rows p (1 - p)))), rounded up to the 64 the head rounds to anyway.  A step that still overflows
    drops the last labelled rows, visibly: model.transformer.mlm_counts[1] counts them."""
    import math
    rows, p = int(rows), float(p)
    if rows < 1 or not 0.0 <= p <= 1.0 or sigmas < 0:
        raise ValueError(f"mlm_capacity: need rows >= 1, 0 <= p <= 1 and sigmas >= 0 (rows {rows}, p {p}, sigmas {sigmas})")
    need = min(rows, math.ceil(rows * p + sigmas * math.sqrt(rows * p * (1.0 - p))))
    return (max(need, 1) + 63) // 64 * 64


# ---- MSRVTT multiple-choice batches ----------------------------------------------------------------------------------------------
def collate_mc(videos, option_ids, option_mask, question_ids, answers=None) -> Dict:
    """The batch of MSRVTTMCCollator.collate_batch (src/datasets/dataset_video_retrieval.py:328-361) from already tokenised options --
    for tasks.mc_clip_logits / inference_retrieval_mc.  ``videos``: B tensors (n_clips*num_frm, 3, H, W) of one shape (or the stacked
    (B, ...) tensor); ``option_ids`` / ``option_mask``: per video the (n_options, L) token ids and attention mask of its candidate
    captions (B tensors of one shape, or stacked (B, n_options, L), or already flat (B*n_options, L)); ``question_ids``: one id per
    video.  Returns visual_inputs (B, n_clips*num_frm, 3, H, W), text_input_ids / text_input_mask (B*n_options, L) -- video v's options
    are rows v*n_options .. --, question_ids, labels None and n_examples_list [1]*B; the reference's ``meta`` (the option strings) is
    omitted.  ``answers`` (the index of each video's right option) is passed through as batch["answers"]: with the question ids it is
    what the ``id2answer`` of tasks.inference_retrieval_mc is made of."""
    vis = videos if torch.is_tensor(videos) else torch.stack(list(videos))
    bsz = vis.shape[0]
    question_ids = list(question_ids)

    def flat(x):
        x = x if torch.is_tensor(x) else torch.stack(list(x))
        return x.reshape(-1, x.shape[-1]) if x.dim() == 3 else x

    ids, mask = flat(option_ids), flat(option_mask)
    if len(question_ids) != bsz or ids.dim() != 2 or ids.shape != mask.shape or ids.shape[0] % max(bsz, 1) != 0:
        raise ValueError(f"collate_mc: {bsz} videos, {len(question_ids)} question ids, option ids {tuple(ids.shape)}, mask {tuple(mask.shape)}")
    batch = dict(visual_inputs=vis, text_input_ids=ids, text_input_mask=mask, question_ids=question_ids, labels=None,
                 n_examples_list=[1] * bsz)
    if answers is not None:
        answers = [int(a) for a in answers]
        if len(answers) != bsz:
            raise ValueError(f"collate_mc: {len(answers)} answers for {bsz} videos")
        batch["answers"] = answers
    return batch


def collate_qa(videos, text_ids, text_mask, question_ids, labels=None, n_options: int = 1) -> Dict:
    """The tensor half of VideoQACollator.collate_batch (src/datasets/dataset_video_qa.py:193-227) from already tokenised text -- for
    tasks.qa_clip_logits / validate_video_qa, whose loaders hold one question per video.  ``videos``: B tensors (n_clips*num_frm, 3, H,
    W) of one shape (or the stacked tensor); ``text_ids`` / ``text_mask``: per video the (n_options, L) rows "question + option" of the
    multiple-choice tasks (action / transition: n_options = 5) or its one (L,) question (n_options = 1), as B tensors, stacked, or
    already flat (B*n_options, L); ``labels``: one answer per question (the right option, the answer id, or the count) or None, as the
    reference's default_collate of ints gives them (int64).  Returns visual_inputs, text_input_ids / text_input_mask (B*n_options, L),
    question_ids, labels and n_examples_list [1]*B."""
    vis = videos if torch.is_tensor(videos) else torch.stack(list(videos))
    bsz, n_options = vis.shape[0], int(n_options)
    question_ids = list(question_ids)

    def flat(x):
        x = x if torch.is_tensor(x) else torch.stack(list(x))
        return x.reshape(-1, x.shape[-1])

    ids, mask = flat(text_ids), flat(text_mask)
    if len(question_ids) != bsz or ids.shape != mask.shape or ids.shape[0] != bsz * n_options:
        raise ValueError(f"collate_qa: {bsz} videos of {n_options} text rows each, {len(question_ids)} question ids, text ids "
                         f"{tuple(ids.shape)}, mask {tuple(mask.shape)}")
    if labels is not None:
        labels = torch.as_tensor([int(a) for a in labels] if not torch.is_tensor(labels) else labels).reshape(-1)
        if labels.numel() != bsz:
            raise ValueError(f"collate_qa: {labels.numel()} labels for {bsz} questions")
    return dict(visual_inputs=vis, text_input_ids=ids, text_input_mask=mask, question_ids=question_ids, labels=labels,
                n_examples_list=[1] * bsz)


class InfiniteIterator:
    """iterate an iterable object infinitely (src/datasets/dataloader.py:155-175)"""
    def __init__(self, iterable):
        self.iterable = iterable
        self.iterator = iter(iterable)

    def __iter__(self):
        while True:
            try:
                batch = next(self.iterator)
            except StopIteration:
                self.iterator = iter(self.iterable)
                batch = next(self.iterator)
            yield batch


class PrefetchLoader:
    """Drop-in for the reference's PrefetchLoader: iterate it to get batches whose tensors live on ``device``.

    ``img_normalize``: ignored as a callable -- pass the model's pixel statistics at model construction instead (frames are
    delivered as uint8 and normalised inside the stem pack).  (task, batch) tuples of the reference's MetaLoader pass
    through unchanged.  A ``RawFrames`` anywhere in a batch travels as its two tensors (flat bytes, table) through the same slots.

    A batch is handed out only AFTER the consumer's current stream has been made to wait for the event behind its copies (``__iter__``:
    wait_event, record_stream, then yield), so whatever the consumer enqueues on that stream may read the batch where it lies -- a
    captured step's replay reads ``RawFrames.flat`` in place (captured.CapturedStep(raw_frames=True)) and needs nothing more from here."""

    def __init__(self, loader: Iterable, device=None, img_normalize=None, slots: int = 2):
        self.loader = loader
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.img_normalize = img_normalize
        self.slots = max(2, slots)
        self._cuda = self.device.type == "cuda"
        self.stream = torch.cuda.Stream(device=self.device) if self._cuda else None
        self._pinned: Dict = {}           # (key, slot) -> pinned host tensor
        self._slot_free = [None] * self.slots      # event recorded after the slot's last H2D copy
        self._n = 0

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):
        return getattr(self.__dict__["loader"], name)

    # ---- staging ---------------------------------------------------------------------------------------------------------
    def _stage(self, key, slot, t: torch.Tensor) -> torch.Tensor:
        """host tensor -> pinned slot (reallocated when the batch outgrows it) -> device, on the side stream"""
        if not self._cuda:
            return t.to(self.device)
        buf = self._pinned.get((key, slot))
        n = t.numel()
        if buf is None or buf.dtype != t.dtype or buf.numel() < n:
            buf = torch.empty(max(n, 1), dtype=t.dtype).pin_memory()
            self._pinned[(key, slot)] = buf
        view = buf[:n].view(t.shape)
        view.copy_(t)                                   # pageable -> pinned (host memcpy)
        return view.to(self.device, non_blocking=True)  # pinned -> HBM, asynchronous on the side stream

    def _move(self, obj, slot, prefix=""):
        if isinstance(obj, RawFrames):                  # flat bytes and table: two keys of the pinned double buffer
            if obj.source is not None:
                return obj.to(self.device)                  # (raises: an indirect one cannot travel)
            table = obj.table.contiguous()
            host = obj.host_table if obj.host_table is not None else (table if not table.is_cuda else None)
            return obj._with(self._move(obj.flat, slot, f"{prefix}/flat"), self._move(table, slot, f"{prefix}/table"),
                             host.contiguous() if host is not None else None)
        if torch.is_tensor(obj):
            return self._stage(prefix, slot, obj) if obj.device.type == "cpu" else obj.to(self.device, non_blocking=True)
        if isinstance(obj, dict):
            return {k: self._move(v, slot, f"{prefix}/{k}") for k, v in obj.items()}
        if isinstance(obj, (list, tuple)):
            moved = [self._move(v, slot, f"{prefix}/{i}") for i, v in enumerate(obj)]
            return type(obj)(moved) if not hasattr(obj, "_fields") else type(obj)(*moved)
        return obj

    def _preload(self, it) -> Optional[tuple]:
        try:
            batch = next(it)
        except StopIteration:
            return None
        slot = self._n % self.slots
        self._n += 1
        if not self._cuda:
            return self._move(batch, slot), None
        ev_free = self._slot_free[slot]
        if ev_free is not None:
            ev_free.synchronize()                       # the copy that last read this slot's pinned buffers has finished
        with torch.cuda.stream(self.stream):
            moved = self._move(batch, slot)
            ev = torch.cuda.Event()
            ev.record(self.stream)
        self._slot_free[slot] = ev
        return moved, ev

    @staticmethod
    def _record_stream(obj, stream):
        if isinstance(obj, RawFrames):
            for t in (obj.flat, obj.table):
                if t is not None and t.is_cuda:
                    t.record_stream(stream)
        elif torch.is_tensor(obj):
            if obj.is_cuda:
                obj.record_stream(stream)
        elif isinstance(obj, dict):
            for v in obj.values():
                PrefetchLoader._record_stream(v, stream)
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                PrefetchLoader._record_stream(v, stream)

    def __iter__(self) -> Iterator:
        it = iter(self.loader)
        nxt = self._preload(it)
        while nxt is not None:
            batch, ev = nxt
            if ev is not None:
                cur = torch.cuda.current_stream(self.device)
                cur.wait_event(ev)                      # only this batch's copies, not everything queued behind them
                self._record_stream(batch, cur)
            nxt = self._preload(it)                     # batch i+1 travels while batch i computes
            yield batch
