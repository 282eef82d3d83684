"""The task loops as hipGraph replays: shape signatures, static input buffers, a bounded graph cache and a safe eager fallback around
the step that bench.py times.

    stepper = CapturedStep(model, optimizer, cfg)               # tasks.start_training(..., capture=True) builds this
    loss = stepper.step(batch, global_step, n_epoch)            # means what tasks.train_step means on the same arguments

A batch is keyed by its SIGNATURE -- everything that fixes the launch sequence.  The first sight of a signature runs the eager
``tasks.train_step`` (which also fills every host-built cache -- rt.tables, _src_cache, the split-K workspace, the MLM tables -- each of
which would be an illegal H2D copy inside a capture).  The second sight allocates static input buffers, stages the batch into them
with ONE launch (ops.copy_ranges / cb_copy_ranges), captures ``make_step(...).device_step`` over them under ``torch.cuda.graph`` (one
memory pool for all graphs of the object) and then runs this step eagerly once more: a capture executes nothing on the device, so a
capture that raises has applied no part of a step -- parameters, moments and gradients are untouched, the host-side dropout counter is put
back, and the step bookkeeping it touched (lazy zero-grad flags, pending-node counts) is reset by the eager step that follows anyway; the
signature is marked uncapturable.  From the third
sight on: stage, ``set_learning_rates`` + ``optimizer.prepare_step()`` eagerly (fresh host-side hyper-parameters), ``graph.replay()``
(fresh dropout masks and, with the model config's pixel_sampling = "device", a fresh pixel selection, with cfg.mlm_masking = "device" fresh
masked-LM masks: the graph advances the device seed word).  The cache is LRU over ``max_graphs`` entries; an evicted signature is
captured again at its next sight and its static buffers go with its graph.

Nothing is silently frozen into a graph: whatever produces per-step values on the host, or takes its launch geometry from the data,
stays on the eager step, with one warning per signature that names the reason (``CapturedStep._why_eager``).

``mode="dry"`` (``capture="dry"``) does the signature and staging bookkeeping without graphs: a "replay" is the eager step on the static
buffers.  It is how the host logic is tested where no GPU is present.
"""
import warnings
from collections import OrderedDict
from types import SimpleNamespace

import torch

from . import ops


def make_step(model, batch, tcfg, opt, sync, labels, counts, n_clips, frames, pool, fold=True, loss_fn=None):
    """The closures of one training step on prepared objects -- bench.py's default path calls THIS through clipbert_amd.bench.step (its
    `forward_loss`, `host_prepare` and `device_step_single` are these functions), so tests/test_bench_step.py tests what is timed, and
    CapturedStep captures the same `device_step` over its static buffers.  ``loss_fn(model, batch, tcfg)`` replaces the clip stack and
    the pooled loss (tasks.pretrain_loss)."""
    from . import tasks
    state = {"global_step": 0}
    dev = labels.device if labels is not None else model.rt.bank.device
    one = torch.ones((), dtype=torch.float32, device=dev)          # d(loss)/d(loss): persistent, so that backward() launches no fill

    def forward_loss():
        if loss_fn is not None:
            return loss_fn(model, batch, tcfg)
        stack = tasks.forward_clips_stack(model, batch, n_clips, frames, fold=fold, cfg=tcfg)       # (n_clips, pairs, C) logits
        return tasks.training_loss(model, stack, labels, counts, pool)                              # clip pooling (a20) + loss

    def host_prepare():
        """per-step host work of a real training loop: LR schedule onto the 8 groups, hyper-parameter upload"""
        state["global_step"] += 1
        tasks.set_learning_rates(opt, tcfg, state["global_step"])
        opt.prepare_step(grad_scale=sync.grad_scale if sync is not None else 1.0)

    def device_step():
        """everything a 1-GPU step enqueues (capturable)"""
        opt.zero_grad(lazy=True)
        model.rt.begin_step()
        loss = forward_loss()
        loss.backward(one)
        ops.counter_add(model.rt.seed_dev)
        opt.launch()
        return loss

    return SimpleNamespace(forward_loss=forward_loss, host_prepare=host_prepare, device_step=device_step, state=state, one=one)


def _describe(v):
    """what a batch entry contributes to the signature"""
    if torch.is_tensor(v):
        return (str(v.dtype), tuple(v.shape), str(v.device))
    if v is None:
        return None
    return (type(v).__name__, tuple(getattr(v, "shape", ())))


class _Replayer:
    """Signature -> graph bookkeeping shared by CapturedStep and CapturedForward.

    ``stats``: eager (calls that ran the eager code: first sights, capture sights, fallbacks, uncapturable signatures), replays,
    captures, failed_captures, fallbacks, evictions, max_live (most graphs alive at once).  ``log``: "eager" | "replay" per call."""

    def __init__(self, max_graphs: int, mode: str):
        if mode not in ("graph", "dry"):
            raise ValueError(f"mode must be 'graph' or 'dry', not {mode!r}")
        if max_graphs < 1:
            raise ValueError("max_graphs must be at least 1")
        self.max_graphs, self.mode = int(max_graphs), mode
        self.graphs = OrderedDict()                 # signature -> entry(graph, bufs, static, out), least recently used first
        self.seen = {}                              # signature -> eager sights that succeeded
        self.uncapturable = {}                      # signature -> what its capture raised
        self._warned = set()
        self._pool = None
        self.stats = dict(eager=0, replays=0, captures=0, failed_captures=0, fallbacks=0, evictions=0, max_live=0)
        self.log = []

    def _warn(self, sig, reason):
        if sig not in self._warned:
            self._warned.add(sig)
            warnings.warn(f"{type(self).__name__}: {reason}: this signature runs eagerly", RuntimeWarning, stacklevel=4)

    @staticmethod
    def _stage(bufs, tensors):
        """the caller's tensors (on the buffers' device: anything else runs eagerly) into the static buffers, ONE launch"""
        ops.copy_ranges([(buf, tensors[k].contiguous()) for k, buf in bufs.items()])

    def _static(self, others, bufs):
        """(what the captured body is handed, the entry's data.FrameSource or None)"""
        return dict(others, **bufs), None

    def _stage_entry(self, entry, tensors):
        self._stage(entry.bufs, tensors)

    def _off_device(self, tensors):
        """the fallback reason for a tensor that is not where the model is (a graph would run it elsewhere than the eager step does)"""
        dev = self._device()
        for k, v in tensors.items():
            if v.device != dev:
                return f"{k} is on {v.device}, the model on {dev}"
        return None

    def _run(self, sig, tensors, others, reason, eager):
        if reason is not None:
            self._warn(sig, reason)
            self.stats["fallbacks"] += 1
        if reason is not None or sig in self.uncapturable:
            self.stats["eager"] += 1
            self.log.append("eager")
            return eager()
        entry = self.graphs.get(sig)
        if entry is not None:
            self.graphs.move_to_end(sig)
            self._stage_entry(entry, tensors)
            out = self._replay(entry)
            self.stats["replays"] += 1
            self.log.append("replay")
            return out
        n = self.seen.get(sig, 0)
        if n >= 1:
            self._capture(sig, tensors, others)
        out = eager()
        self.seen[sig] = n + 1
        self.stats["eager"] += 1
        self.log.append("eager")
        return out

    def _capture(self, sig, tensors, others):
        dev = self._device()
        bufs = {k: torch.empty(v.shape, dtype=v.dtype, device=dev) for k, v in tensors.items()}
        static, source = self._static(others, bufs)
        entry = SimpleNamespace(graph=None, bufs=bufs, static=static, source=source, out=None, body=self._body(static))
        self._stage_entry(entry, tensors)
        if self.mode == "graph":
            if self._pool is None:
                self._pool = torch.cuda.graph_pool_handle()
            graph = torch.cuda.CUDAGraph()
            rt = self.model.rt
            fwd = rt.forward_count                      # the host half of the dropout seeds: the eager steps go on counting as if no capture happened
            try:
                # (thread_local: a runtime call from ANOTHER thread, e.g. a loader pinning memory, does not fail this capture)
                with torch.cuda.graph(graph, pool=self._pool, capture_error_mode="thread_local"):
                    entry.out = entry.body()
            except Exception as e:                      # host exception: the capture has ended (torch.cuda.graph's exit), nothing was executed
                rt.forward_count = fwd
                self.uncapturable[sig] = f"{type(e).__name__}: {e}"     # (the text only: the exception's traceback would keep the capture's tensors alive)
                self.stats["failed_captures"] += 1
                del graph
                warnings.warn(f"{type(self).__name__}: capture failed ({type(e).__name__}: {e}): this signature runs eagerly",
                              RuntimeWarning, stacklevel=4)
                return
            rt.forward_count = fwd
            entry.graph = graph
        self.stats["captures"] += 1
        self.graphs[sig] = entry
        while len(self.graphs) > self.max_graphs:
            self.graphs.popitem(last=False)             # graph + static buffers die with the entry
            self.stats["evictions"] += 1
        self.stats["max_live"] = max(self.stats["max_live"], len(self.graphs))


class CapturedStep(_Replayer):
    """``step(batch, global_step, n_epoch=0) -> loss`` (detached, on the device): tasks.train_step on the same arguments, replayed from
    a captured hipGraph once the batch's signature has been seen twice (module docstring).

    Signature: dtype, shape and device of every tensor of the batch and which optional keys are present; tuple(n_examples_list);
    cfg.train_n_clips, num_frm, score_agg_func, task, num_labels; model.training; for pretraining cfg.mlm_rows, mlm_capacity, use_mlm,
    use_itm, mlm_masking, mlm_probability; fold_clips; pixel_sampling and pixel_random_sampling_size of the config the encoder reads.

    ``pad_text_to`` (e.g. cfg.max_txt_len): text_input_ids / text_input_mask (and mlm_labels, with -100) are right-padded to that many
    columns with pad id 0 and mask 0 before the signature is taken, so that the text length of a batch stops multiplying signatures
    (two torch pads per step; a collate function that pads to a fixed length costs nothing).  Padded keys are masked out of the
    attention, so results then differ from the un-padded eager step only by the order of the floating-point sums in attention (its
    key tiles shift); eager sights and fallbacks run on the padded batch too.

    ``raw_frames=True`` (tasks.start_training: cfg.capture_raw_frames): data.RawFrames batches replay too.  Such an entry contributes
    its leading shape, max_img_size, hwc, pixfmt, matrix and device to the signature -- NOT its byte count or any table value: batches of
    other native resolutions replay from the same graph.  Per signature the static state is an (n_frames, 5) table buffer, filled by the
    staging launch of the text tensors, and one descriptor (data.FrameSource: a pinned two-slot upload guarded by events, never
    captured); the captured body sees the indirect RawFrames over the two, whose launches (cb_resize_pack_u8_src / _yuv420_src) read
    address and size of the batch's ``flat`` from the descriptor: the pixel bytes are read where the loader put them, never copied.
    Every step, replays included, first runs ops.resize_table_check on the batch's host table against the batch's own byte count and
    raises what the eager step's launch would have raised -- before anything is staged or replayed.  The stepper holds the staged
    batch's ``flat`` until the next batch of that signature has been staged (or the entry is evicted); descriptor upload, staging and
    replay are ordered on the current stream.  ``mode="dry"`` does the same and runs the eager step on the indirect RawFrames.

    Runs eagerly, with one warning per signature: a gradient exchange (``sync`` with several ranks or its loopback),
    cfg.gradient_accumulation_steps > 1, a data.RawFrames batch without ``raw_frames=True`` (nothing re-points a graph's frozen buffer
    argument), and with it: one without a host table (its rows could not be checked before a replay), one whose ``flat`` or ``table``
    is not on the model's device, one that is indirect already; config.
    pixel_random_sampling_size > 0 in training with pixel_sampling = "host" (numpy draws the selection per forward; "device" draws it
    inside the graph with cb_pixel_sample, seeded like the dropout masks), the labelled-rows masked-LM head without a fixed
    cfg.mlm_capacity (whether the batch carries the labels or cfg.mlm_masking = "device" draws them inside the step with cb_mlm_mask: the
    count of labelled rows is then binomial, data.mlm_capacity sizes the slots; otherwise a device-masked pretraining step is captured like
    any other and every replay masks afresh -- ``pad_text_to`` pads with the pad id, which is never labelled), non-tensor batch entries the model reads, batch tensors that are not on the model's device (a loader that left them
    on the host), and a signature whose capture raised."""

    RAW_TABLE = "visual_inputs.table"              # the key of a RawFrames batch's table among the staged tensors

    def __init__(self, model, optimizer, cfg, loss_fn=None, fold_clips=True, max_graphs=8, pad_text_to=None, sync=None, mode="graph",
                 raw_frames=False):
        super().__init__(max_graphs, mode)
        self.model, self.optimizer, self.cfg, self.loss_fn, self.fold_clips, self.sync = model, optimizer, cfg, loss_fn, fold_clips, sync
        self.pad_text_to = int(pad_text_to) if pad_text_to else None
        self.raw_frames = bool(raw_frames)
        self._raw = None                            # the RawFrames of the batch being stepped, when it takes the replay path

    def _device(self):
        return self.model.rt.bank.device

    # ---- what fixes the launch sequence -----------------------------------------------------------------------------------------
    def _encoder_config(self):
        """the config object the encoder reads (pixel sub-sampling keys)"""
        return getattr(getattr(self.model.transformer, "bert", None), "config", self.model.config)

    def signature(self, batch):
        from .tasks import _get
        cfg, enc_cfg = self.cfg, self._encoder_config()
        entries = tuple(sorted((k, self._describe_entry(v)) for k, v in batch.items() if k != "n_examples_list"))
        return (entries, tuple(batch["n_examples_list"]), _get(cfg, "train_n_clips", 1), _get(cfg, "num_frm"), _get(cfg, "score_agg_func", "mean"),
                _get(cfg, "task"), _get(cfg, "num_labels"), bool(self.model.training), _get(cfg, "mlm_rows", "labelled"), _get(cfg, "mlm_capacity"),
                _get(cfg, "use_mlm", True), _get(cfg, "use_itm", True), bool(self.fold_clips),
                getattr(enc_cfg, "pixel_sampling", "host") or "host", int(getattr(enc_cfg, "pixel_random_sampling_size", 0) or 0),
                _get(cfg, "mlm_masking", "host") or "host", _get(cfg, "mlm_probability", 0.15))

    def _describe_entry(self, v):
        from .data import RawFrames
        if self.raw_frames and isinstance(v, RawFrames):
            # what fixes the launches: neither the byte count nor any table value -- other native resolutions replay from the same graph
            return ("RawFrames", tuple(v.table.shape[:-1]), v.max_img_size, v.hwc, v.pixfmt, v.matrix, str(v.device))
        return _describe(v)

    def _why_eager_raw(self, rf):
        """a RawFrames batch under raw_frames=True: why it cannot be replayed, or None"""
        if rf.source is not None:
            return "RawFrames batch that is indirect already (its descriptor is the caller's to point)"
        if rf.host_table is None:
            return "RawFrames batch without a host table (its rows cannot be checked before a replay)"
        return self._off_device({"visual_inputs.flat": rf.flat, "visual_inputs.table": rf.table})

    def _why_eager(self, batch):
        from .data import RawFrames
        from .tasks import _SKIP_KEYS, _get
        cfg = self.cfg
        if self.sync is not None and self.sync.active:
            return "gradient exchange between ranks (sync)"
        if int(_get(cfg, "gradient_accumulation_steps", 1) or 1) > 1:
            return "gradient_accumulation_steps > 1"
        if isinstance(batch.get("visual_inputs"), RawFrames):
            if not self.raw_frames:
                return "RawFrames batch (launch geometry from its host table)"
            reason = self._why_eager_raw(batch["visual_inputs"])
            if reason is not None:
                return reason
        enc_cfg = self._encoder_config()
        if (self.model.training and int(getattr(enc_cfg, "pixel_random_sampling_size", 0) or 0) > 0
                and (getattr(enc_cfg, "pixel_sampling", "host") or "host") != "device"):
            return "pixel_random_sampling_size > 0 (the selection is drawn on the host per forward; pixel_sampling = 'device' draws it in the graph)"
        # (labels the batch carries, or labels tasks._pretrain_forward draws on the device: only the pretraining config has the key)
        drawn = (_get(cfg, "mlm_masking", "host") or "host") == "device" and bool(_get(cfg, "use_mlm", True))
        if ((batch.get("mlm_labels") is not None or drawn) and _get(cfg, "mlm_rows", "labelled") == "labelled"
                and _get(cfg, "mlm_capacity") is None):
            return "labelled-rows masked-LM head without a fixed mlm_capacity"
        for k, v in batch.items():
            if not torch.is_tensor(v) and v is not None and k not in _SKIP_KEYS:
                return f"batch[{k!r}] is a {type(v).__name__}, not a tensor"
        return self._off_device({k: v for k, v in batch.items() if torch.is_tensor(v)})

    def _pad(self, batch):
        lt = batch["text_input_ids"].shape[1]
        if self.pad_text_to is None or lt == self.pad_text_to:
            return batch
        if lt > self.pad_text_to:
            raise ValueError(f"pad_text_to = {self.pad_text_to} but the batch has {lt} text columns")
        pad = (0, self.pad_text_to - lt)
        out = dict(batch)
        for k, fill in (("text_input_ids", int(getattr(self.model.config, "pad_token_id", 0) or 0)), ("text_input_mask", 0), ("mlm_labels", -100)):
            if torch.is_tensor(batch.get(k)):
                out[k] = torch.nn.functional.pad(batch[k], pad, value=fill)
        return out

    # ---- the step --------------------------------------------------------------------------------------------------------------
    def _grad_scale(self):
        return self.sync.grad_scale if self.sync is not None else 1.0

    def _body(self, static):
        from . import tasks
        cfg = self.cfg
        if self.mode == "dry":
            return None
        fns = make_step(self.model, static, cfg, self.optimizer, self.sync, static.get("labels"), static["n_examples_list"],
                        tasks._get(cfg, "train_n_clips", 1), tasks._get(cfg, "num_frm"), tasks._get(cfg, "score_agg_func", "mean"),
                        fold=self.fold_clips, loss_fn=self.loss_fn)
        return fns.device_step

    def _static(self, others, bufs):
        from .data import FrameSource, RawFrames
        static, rf = dict(others, **bufs), self._raw
        if rf is None:
            return static, None
        # the body sees an indirect RawFrames over the static table and ONE descriptor: both keep their addresses, step() refills them
        source = FrameSource(self._device())
        table = static.pop(self.RAW_TABLE).view(*rf.table.shape)
        static["visual_inputs"] = RawFrames.indirect(source.desc, table, rf.max_img_size, rf.hwc, None, rf.pixfmt, rf.matrix)
        return static, source

    def _stage_entry(self, entry, tensors):
        """descriptor, then the ONE staging launch, both on the stream the replay follows on; the entry holds the batch's ``flat`` from
        here until the next batch of its signature is staged (or the entry is evicted): a replay reads it where it lies"""
        if entry.source is not None:
            entry.source.point_at(self._raw.flat)
        self._stage(entry.bufs, tensors)

    def _replay(self, entry):
        from . import tasks
        if entry.graph is None:                         # dry: the eager step on the static buffers
            return tasks.train_step(self.model, self.optimizer, entry.static, self.cfg, self._at[0], sync=self.sync, n_epoch=self._at[1],
                                    fold_clips=self.fold_clips, loss_fn=self.loss_fn)
        tasks.set_learning_rates(self.optimizer, self.cfg, self._at[0] + 1, self._at[1])
        self.optimizer.prepare_step(grad_scale=self._grad_scale())
        entry.graph.replay()
        return entry.out.detach().clone()               # (the pool is shared: the next replay of any graph may reuse the loss's memory)

    def step(self, batch, global_step, n_epoch=0, micro_step=0):
        from . import tasks
        from .data import RawFrames
        batch = self._pad(batch)
        reason = self._why_eager(batch)
        sig = self.signature(batch)
        self._at = (global_step, n_epoch)
        tensors = {k: v for k, v in batch.items() if torch.is_tensor(v)}
        others = {k: (list(v) if k == "n_examples_list" else v) for k, v in batch.items() if not torch.is_tensor(v)}
        rf = batch.get("visual_inputs")
        self._raw = rf if self.raw_frames and reason is None and isinstance(rf, RawFrames) else None
        if self._raw is not None:
            # every step, replays included, BEFORE anything is staged or replayed: the rows against this batch's own byte count -- what the
            # eager step's launch would have refused is refused here, in its words (a replay calls no validating entry point)
            table, host = rf.packed_table()
            ops.resize_table_check(host, rf.n_frames, rf.flat.numel(), rf.max_img_size, rf.pixfmt)
            tensors[self.RAW_TABLE] = table             # 40 bytes per frame, in the staging launch of the text tensors
            del others["visual_inputs"]

        def eager():
            return tasks.train_step(self.model, self.optimizer, batch, self.cfg, global_step, sync=self.sync, n_epoch=n_epoch,
                                    micro_step=micro_step, fold_clips=self.fold_clips, loss_fn=self.loss_fn)

        try:
            return self._run(sig, tensors, others, reason, eager)
        finally:
            self._raw = None                            # (only the staged entry keeps the batch's bytes alive)


class CapturedForward(_Replayer):
    """The same machinery without backward or optimizer around ``model.forward_from_grid`` (no_grad, eval): the encoder passes of
    tasks.inference_retrieval_video.  ``logits(grid, ids, mask, n_examples_list) -> logits`` (a fresh tensor); the signature is the
    dtype / shape / device of the three tensors -- i.e. (clips, captions, text length, grid shape) -- and the counts: one full and one
    remainder signature per video set."""

    def __init__(self, model, max_graphs=8, mode="graph"):
        super().__init__(max_graphs, mode)
        self.model = model

    def _device(self):
        return self.model.rt.bank.device

    def _forward(self, b):
        return self.model.forward_from_grid(dict(visual_inputs=b["visual_inputs"], text_input_ids=b["text_input_ids"],
                                                 text_input_mask=b["text_input_mask"], labels=None,
                                                 n_examples_list=list(b["n_examples_list"])))["logits"]

    def _body(self, static):
        return lambda: self._forward(static)

    def _replay(self, entry):
        if entry.graph is None:
            return entry.body()
        entry.graph.replay()
        return entry.out.clone()

    @torch.no_grad()
    def logits(self, grid, ids, mask, n_examples_list):
        if self.model.training:
            raise RuntimeError("CapturedForward is for inference: model.eval() first")
        tensors = dict(visual_inputs=grid, text_input_ids=ids, text_input_mask=mask)
        others = dict(n_examples_list=list(n_examples_list))
        sig = (tuple(sorted((k, _describe(v)) for k, v in tensors.items())), tuple(n_examples_list))
        return self._run(sig, tensors, others, self._off_device(tensors), lambda: self._forward(dict(tensors, **others)))
