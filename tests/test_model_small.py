"""End-to-end ClipBert forward + backward (CNN trunk, cross-modal encoder, heads, losses) through the
product Python layer against the CPU oracle and its autograd gradients.  Small widths / 2 layers /
64x128 frames keep the host-emulator run to seconds; the same cases run on the GPU (marked `gpu`), and
the full-size parity runs live in test_gpu_full.py."""
import numpy as np
import pytest
import torch

import dropout_restatement as DR
import parity_bounds as PB
from clipbert_amd import modeling as M
from clipbert_amd import synthetic as S
from clipbert_amd.modeling import runtime as RT
from oracle import clipbert_oracle as O

SMALL = dict(O.BASE_CONFIG, hidden_size=128, num_attention_heads=2, intermediate_size=256, num_hidden_layers=2,
             vocab_size=200, max_position_embeddings=32, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)

HEAD_CLS = dict(retrieval=M.ClipBertForVideoTextRetrieval, multiple_choice=M.ClipBertForMultipleChoice,
                sequence_classification=M.ClipBertForSequenceClassification, pretraining=M.ClipBertForPreTraining,
                regression=M.ClipBertForRegression)


_SD_CACHE = {}


def _state_dict(cfg, head, seed):
    """synthetic weights are deterministic per (config, head, seed): generate once per process (callers never mutate them)"""
    key = (head, seed, tuple(sorted((k, str(v)) for k, v in cfg.items())))
    if key not in _SD_CACHE:
        _SD_CACHE[key] = S.full_state_dict(cfg, head, seed)
    return _SD_CACHE[key]


def build(head, extra, dtype, dev, seed=5):
    cfg = dict(SMALL, **extra)
    sd = _state_dict(cfg, head, seed)
    model = M.ClipBert(cfg, detectron2_model_cfg="R-50-grid.yaml", transformer_cls=HEAD_CLS[head])
    missing, unexpected = model.load_state_dict(sd, strict=True)
    model.to(dev).eval()
    model.prepare(dtype=dtype, device=dev)
    return cfg, sd, model


def to_dev(batch, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}


def make_batch(cfg, head, n_videos, repeat, lt, seed=5):
    frames = S.synthetic_frames(n_videos, 2, 64, seed)[..., :64, :].repeat(1, 1, 1, 1, 2)   # (Bv, 2, 3, 64, 128)
    frames = frames.contiguous()
    ids, mask = S.synthetic_text(n_videos * repeat, lt, seed, cfg["vocab_size"])
    ids = ids.clamp(max=cfg["vocab_size"] - 1)
    batch = dict(visual_inputs=O.image_norm(frames, S.PIXEL_MEAN, S.PIXEL_STD), text_input_ids=ids, text_input_mask=mask,
                 n_examples_list=[repeat] * n_videos)
    return batch


def grads_of_oracle(sd, batch, cfg, head, loss_fn):
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k) for k, v in sd.items()}
    if head == "pretraining":      # tied weights share one leaf
        sdr["transformer.cls.predictions.decoder.weight"] = sdr["transformer.bert.embeddings.word_embeddings.weight"]
        sdr["transformer.cls.predictions.decoder.bias"] = sdr["transformer.cls.predictions.bias"]
    out = O.clipbert_forward(sdr, batch, cfg, head)
    loss_fn(out).backward()
    return out, sdr


def forward_tol(hw):
    # the emulator shares the host libm with the oracle; on the GPU erf/exp/tanh differ in the last ulps
    return dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)


def assert_grads_match_oracle(hw, model, sdr):
    """every trainable parameter's gradient against the oracle's autograd (the leaves of ``sdr``)"""
    gt = 2e-3 if hw.name == "emul" else 5e-3
    checked = 0
    worst = (0.0, "")
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        g_ref = sdr[name].grad
        if g_ref is None:
            g_ref = torch.zeros_like(p, device="cpu")
        scale = max(g_ref.abs().max().item(), 1e-5)   # key.bias has an exactly-zero gradient (softmax shift invariance)
        diff = p.grad.cpu() - g_ref
        err = diff.abs().max().item() / scale
        if err > worst[0]:
            worst = (err, name)
        if hw.name == "emul":
            assert err < gt, f"{name}: relative grad error {err:.3e} (|g|max {scale:.3e})"
        else:
            # On the GPU exp/erf/tanh and the summation orders differ from the host in the last ulps; a pre-activation
            # within that distance of zero flips its ReLU (or a max-pool tie) and changes a handful of gradient
            # elements by a finite amount.  So: tight bound on the relative L2 error of the whole tensor, loose bound
            # on the single worst element.
            l2 = diff.norm().item() / max(g_ref.norm().item(), 1e-5 * g_ref.numel() ** 0.5)
            assert l2 < gt, f"{name}: relative L2 grad error {l2:.3e} (|g| {g_ref.norm().item():.3e})"
            assert err < 10 * gt, f"{name}: worst-element grad error {err:.3e} (|g|max {scale:.3e})"
        checked += 1
    assert checked > 40, checked
    # frozen stem / res2 must not have been touched
    assert model.cnn.feature.backbone.stem.conv1.weight.grad is None


@pytest.mark.parametrize("head,extra,repeat", [
    ("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), 2),
    ("pretraining", dict(), 1),
])
def test_forward_backward_matches_oracle_fp32(hw, head, extra, repeat):
    torch.manual_seed(0)
    cfg, sd, model = build(head, extra, torch.float32, hw.dev)
    n_videos, lt = 2, 6
    batch = make_batch(cfg, head, n_videos, repeat, lt)
    n_pairs = n_videos * repeat
    if head == "pretraining":
        mlm = batch["text_input_ids"].clone()
        mlm[:, ::2] = -100
        batch["mlm_labels"] = mlm
        batch["itm_labels"] = S.synthetic_labels(n_pairs, 2, 5)
        loss_fn = lambda o: o["mlm_loss"].mean() + o["itm_loss"].mean()
    else:
        batch["labels"] = S.synthetic_labels(n_pairs, 2, 5)
        loss_fn = lambda o: o["loss"].mean()
    ref, sdr = grads_of_oracle(sd, batch, cfg, head, loss_fn)
    out = model(to_dev(batch, hw.dev))
    ft = forward_tol(hw)
    if head == "pretraining":
        torch.testing.assert_close(out["itm_scores"].cpu(), ref["itm_scores"], **ft)
        torch.testing.assert_close(out["mlm_scores"].cpu(), ref["mlm_scores"], **ft)
        torch.testing.assert_close(out["mlm_loss"].cpu(), ref["mlm_loss"], **ft)
    else:
        torch.testing.assert_close(out["logits"].cpu(), ref["logits"], **ft)
        torch.testing.assert_close(out["loss"].cpu(), ref["loss"], **ft)
    model.rt.bank.zero_grad()
    loss_fn(out).backward()
    assert_grads_match_oracle(hw, model, sdr)


# ---- model.train(): every dropout site on, held to the oracle through masks restated from csrc/common.h (tests/dropout_restatement.py) ----
_SITES = dict(emb=RT._SITE_EMB, attn=RT._SITE_ATTN, self_out=RT._SITE_SELF_OUT, out=RT._SITE_OUT, pool=RT._SITE_POOL, reg=RT._SITE_REG)
RETRIEVAL_CE = dict(num_labels=2, loss_type="ce", margin=0.1)


def restated_masks(cfg, fwd_i, seed_word):
    """the hook of O.dropout_masks that drops what the product drops in its fwd_i-th training forward.  The product as it is: the
    regression head's second dropout reads rt.forward_count AFTER the encoder advanced it."""
    def fn(site, layer, x):
        p = cfg["attention_probs_dropout_prob"] if site == "attn" else cfg["hidden_dropout_prob"]
        f = fwd_i + 1 if site == "reg" else fwd_i
        return x * DR.site_mask(_SITES[site], layer, f, seed_word, x.shape, p, dtype=x.dtype)
    return fn


def oracle_leaves(sd, head):
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k and "running" not in k) for k, v in sd.items()}
    if head == "pretraining":      # tied weights share one leaf
        sdr["transformer.cls.predictions.decoder.weight"] = sdr["transformer.bert.embeddings.word_embeddings.weight"]
        sdr["transformer.cls.predictions.decoder.bias"] = sdr["transformer.cls.predictions.bias"]
    return sdr


def train_case(cfg, head, repeat, seed=5):
    """(batch, loss_fn, names of the outputs the forward is compared on) of one head in training"""
    # two videos: with the third one of test_regression_head_matches_oracle a ReLU pre-activation of res3.2.conv1 lies 4e-5 from zero,
    # fp32 summation order flips it, and the res3 weight gradients move by 1e-2 of their largest element with dropout off as well
    n_videos = 2
    batch = make_batch(cfg, head, n_videos, repeat, 6, seed)
    n_pairs = n_videos * repeat
    if head == "pretraining":
        mlm = batch["text_input_ids"].clone()
        mlm[:, ::2] = -100
        batch["mlm_labels"] = mlm
        batch["itm_labels"] = S.synthetic_labels(n_pairs, 2, seed)
        return batch, (lambda o: o["mlm_loss"].mean() + o["itm_loss"].mean()), ("itm_scores", "mlm_scores", "mlm_loss")
    if head == "regression":
        batch["labels"] = torch.tensor([1.0, 4.0, 2.0, 7.0])
    else:
        batch["labels"] = S.synthetic_labels(n_pairs, 2, seed)
    return batch, (lambda o: o["loss"].mean()), ("logits", "loss")


def oracle_batch(batch, head):
    return dict(batch, training=True) if head == "regression" else dict(batch)        # (BatchNorm1d on batch statistics)


TRAIN_CASES = [
    ("retrieval", RETRIEVAL_CE, 2, 0),
    ("retrieval", RETRIEVAL_CE, 2, 0x1234567890ABCDEF),            # every kernel family adds *seed_ptr to its seed
    ("pretraining", dict(), 1, 0),                                   # (pixel_random_sampling_size unset; no pooled dropout)
    ("regression", dict(num_labels=1, loss_type="mse"), 2, 0),       # training BatchNorm1d, the head's second dropout
]


@pytest.mark.parametrize("head,extra,repeat,seed_word", TRAIN_CASES)
def test_train_mode_forward_backward_matches_masked_oracle_fp32(hw, head, extra, repeat, seed_word):
    """model.train() with p = 0.1 at every site: logits, losses and ALL parameter gradients against the oracle with the restated masks
    at the reference's dropout places (O.dropout_masks) -- same assertions and tolerances as the eval-mode test above.  A wrong mask
    address, a wrong order of bias / activation / dropout / residual, a backward that regenerates another mask, a site too many or
    too few: each costs O(1) per element against tolerances of 1e-3."""
    cfg, sd, model = build(head, extra, torch.float32, hw.dev)
    model.train()
    fwd_i = 3
    model.rt.forward_count = fwd_i
    model.rt.seed_dev.fill_(seed_word)
    batch, loss_fn, outs = train_case(cfg, head, repeat)
    sdr = oracle_leaves(sd, head)
    with O.dropout_masks(restated_masks(cfg, fwd_i, seed_word)):
        ref = O.clipbert_forward(sdr, oracle_batch(batch, head), cfg, head)
    loss_fn(ref).backward()
    ft = forward_tol(hw)
    # the check must not pass with dropout silently off on both sides: the oracle's own train-mode output is far from its eval-mode one.
    # A statement about the oracle alone, so it is made once, against the forward tolerance of the emulator run (for the retrieval
    # logits: 6e-3 .. 1e-2 against 1.4e-4); the same move is 5 .. 13 x the wider tolerance of the GPU run, and is printed.
    with torch.no_grad():
        ref_eval = O.clipbert_forward(sd, oracle_batch(batch, head), cfg, head)

    def moved(t):
        return max(float(((ref[k].detach() - ref_eval[k]).abs() / (t["atol"] + t["rtol"] * ref_eval[k].abs())).max()) for k in outs if "loss" not in k)
    print(f"[train vs eval oracle] {head}: largest move of an output = {moved(dict(rtol=1e-3, atol=1e-4)):.1f} x the emulator run's forward "
          f"tolerance, {moved(ft):.1f} x this run's")
    assert moved(dict(rtol=1e-3, atol=1e-4)) >= 10
    assert moved(ft) >= 3                                        # (a wider tolerance of this run must not swallow the dropout signal)
    out = model(to_dev(batch, hw.dev))
    assert model.rt.forward_count == fwd_i + 1
    for k in outs:
        torch.testing.assert_close(out[k].cpu(), ref[k].detach(), **ft)
    model.rt.bank.zero_grad()
    loss_fn(out).backward()
    assert_grads_match_oracle(hw, model, sdr)


def test_two_train_forwards_one_backward_match_masked_oracle(hw):
    """the timed step's pattern (n_clips forwards, then ONE backward): two training forwards of different inputs, the losses summed,
    one backward -- each forward's backward must regenerate ITS masks (fwd_i and fwd_i + 1 in the oracle)."""
    head = "retrieval"
    cfg, sd, model = build(head, RETRIEVAL_CE, torch.float32, hw.dev)
    model.train()
    fwd_i = 7
    model.rt.forward_count = fwd_i
    sdr = oracle_leaves(sd, head)
    cases = [train_case(cfg, head, 2, seed) for seed in (5, 6)]
    assert not torch.equal(cases[0][0]["text_input_ids"], cases[1][0]["text_input_ids"])
    ref_loss, refs = 0, []
    for i, (batch, loss_fn, _) in enumerate(cases):
        with O.dropout_masks(restated_masks(cfg, fwd_i + i, 0)):
            refs.append(O.clipbert_forward(sdr, dict(batch), cfg, head))
        ref_loss = ref_loss + loss_fn(refs[-1])
    ref_loss.backward()
    model.rt.bank.zero_grad()
    loss = 0
    for (batch, loss_fn, _), ref in zip(cases, refs):
        out = model(to_dev(batch, hw.dev))
        torch.testing.assert_close(out["logits"].cpu(), ref["logits"].detach(), **forward_tol(hw))
        loss = loss + loss_fn(out)
    assert model.rt.forward_count == fwd_i + 2
    loss.backward()
    assert_grads_match_oracle(hw, model, sdr)


def test_train_mode_bf16_gradients_within_the_masked_oracle_yardstick(hw):
    """bf16 model.train() (the benchmarked arithmetic, dropout on) against autograd through the masked fp32 oracle: one-minus-cosine of
    the flat gradient and median per-tensor relative L2 (the figures of test_bench_step.py) held to PB.FACTOR x what the masked oracle
    itself shows in its bf16-storage modes on the same batch with the same masks."""
    head = "retrieval"
    cfg, sd, model = build(head, RETRIEVAL_CE, torch.bfloat16, hw.dev)
    model.train()
    fwd_i, seed_word = 2, 99
    model.rt.forward_count = fwd_i
    model.rt.seed_dev.fill_(seed_word)
    batch, loss_fn, _ = train_case(cfg, head, 2)
    names = [name for name, p in model.named_parameters() if p.requires_grad]

    def oracle_grads(mode):
        sdr = oracle_leaves(sd, head)
        with O.precision(mode), O.dropout_masks(restated_masks(cfg, fwd_i, seed_word)):
            loss = loss_fn(O.clipbert_forward(sdr, dict(batch), cfg, head))
        loss.backward()
        return {n: (sdr[n].grad if sdr[n].grad is not None else torch.zeros_like(sdr[n])).double() for n in names}

    def figures(grads, ref):
        dot = n1 = n2 = 0.0
        per = {}
        for name, r in ref.items():
            g = grads[name]
            dot += float((g * r).sum()); n1 += float((g * g).sum()); n2 += float((r * r).sum())
            if float(r.norm()) > 1e-8:
                per[name] = float((g - r).norm() / r.norm())
        return 1.0 - dot / (n1 ** 0.5 * n2 ** 0.5), float(np.median(list(per.values())))

    ref = oracle_grads("fp32")
    yard = [figures(oracle_grads(m), ref) for m in PB.MODES]
    y_omc, y_med = max(y[0] for y in yard), max(y[1] for y in yard)
    model.rt.bank.zero_grad()
    loss_fn(model(to_dev(batch, hw.dev))).backward()
    params = dict(model.named_parameters())
    omc, med = figures({n: params[n].grad.detach().cpu().double() for n in names}, ref)
    rec = dict(one_minus_cosine=omc, median_tensor_rel_l2=med, tensors=len(ref), yardstick_one_minus_cosine=y_omc, yardstick_median=y_med,
               yardstick_modes=dict(zip(PB.MODES, yard)))
    print(f"[train-mode bf16 vs masked oracle autograd, {hw.name}]", rec)
    assert omc <= PB.FACTOR * y_omc, rec
    assert med <= PB.FACTOR * y_med, rec


def test_bf16_mode_close(hw):
    cfg, sd, model = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), torch.bfloat16, hw.dev)
    batch = make_batch(cfg, "retrieval", 1, 2, 5)
    batch["labels"] = torch.tensor([1, 0])
    with torch.no_grad():
        ref = O.clipbert_forward(sd, batch, cfg, "retrieval")
        out = model(to_dev(batch, hw.dev))
    assert (out["logits"].cpu() - ref["logits"]).abs().max() < 5e-2
    assert (out["loss"].cpu() - ref["loss"]).abs().max() < 5e-2


def test_ragged_examples_and_long_sequence(hw):
    """n_examples_list with different counts per video (repeat_tensor_rows, data_utils.py:344-357, fused into the visual
    embedding gather) and a text long enough that L > 64 (generic attention kernels instead of the one-block MFMA ones)."""
    cfg, sd, model = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1, max_position_embeddings=80), torch.float32, hw.dev)
    frames = S.synthetic_frames(3, 2, 64, 9)[..., :64, :].repeat(1, 1, 1, 1, 2).contiguous()
    counts = [1, 3, 2]
    for lt in (5, 70):
        ids, mask = S.synthetic_text(sum(counts), lt, 9, cfg["vocab_size"])
        ids = ids.clamp(max=cfg["vocab_size"] - 1)
        batch = dict(visual_inputs=O.image_norm(frames, S.PIXEL_MEAN, S.PIXEL_STD), text_input_ids=ids, text_input_mask=mask,
                     n_examples_list=list(counts), labels=S.synthetic_labels(sum(counts), 2, 9))
        with torch.no_grad():
            ref = O.clipbert_forward(sd, dict(batch, n_examples_list=list(counts)), cfg, "retrieval")
            out = model(to_dev(dict(batch, n_examples_list=list(counts)), hw.dev))
        tol = dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)
        torch.testing.assert_close(out["logits"].cpu(), ref["logits"], **tol)
        torch.testing.assert_close(out["loss"].cpu(), ref["loss"], **tol)


def test_backward_cut_at_grid_features(hw):
    """The DP replay plan of bench.py cuts the backward at the grid features (autograd.grad to the grid, then
    grid.backward): same gradients as one loss.backward()."""
    cfg, sd, model = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), torch.float32, hw.dev)
    batch = make_batch(cfg, "retrieval", 2, 2, 6)
    batch["labels"] = S.synthetic_labels(4, 2, 5)
    bank = model.rt.bank
    bank.zero_grad()
    out = model(to_dev(dict(batch, n_examples_list=[2, 2]), hw.dev))
    out["loss"].mean().backward()
    ref = bank.grad.clone()
    bank.zero_grad()
    b = to_dev(dict(batch, n_examples_list=[2, 2]), hw.dev)
    grid = model.grid_features(b["visual_inputs"])
    b["visual_inputs"] = grid
    out = model.forward_from_grid(b)
    (dgrid,) = torch.autograd.grad(out["loss"].mean(), [grid])
    enc_only = bank.grad.clone()
    grid.backward(dgrid)
    torch.testing.assert_close(bank.grad, ref, rtol=1e-5, atol=1e-7)
    t_end = bank.group_range[3][1]
    assert enc_only[t_end:].abs().max() == 0 and (bank.grad[t_end:].abs().max() > 0)      # the CNN part came from phase two
    # ... and the ResNet backward itself in two steps (bench.py's four-graph plan drives modeling.cnn_backward_steps by hand): at
    # its single yield every gradient of grid_encoder and res5 is FINAL -- the data-parallel exchange of those ranges may start --
    # while res3 / res4 have not been touched yet
    bank.zero_grad()
    b = to_dev(dict(batch, n_examples_list=[2, 2]), hw.dev)
    grid = model.grid_features(b["visual_inputs"])
    b["visual_inputs"] = grid
    out = model.forward_from_grid(b)
    (dgrid,) = torch.autograd.grad(out["loss"].mean(), [grid])
    node = grid.grad_fn
    steps = M.cnn_backward_steps(node.bb, node.pack, dgrid.contiguous())
    assert next(steps) == "grid_encoder+res5"
    split = M.cnn_early_split(model)
    mid = bank.group_range[6][0]
    assert t_end < mid < split < bank.n_train
    torch.testing.assert_close(bank.grad[t_end:mid], ref[t_end:mid], rtol=1e-5, atol=1e-7)          # grid_encoder
    torch.testing.assert_close(bank.grad[split:], ref[split:], rtol=1e-5, atol=1e-7)              # res5
    assert bank.grad[mid:split].abs().max() == 0 and ref[mid:split].abs().max() > 0                # res3 + res4: still to come
    assert next(steps, None) is None
    torch.testing.assert_close(bank.grad, ref, rtol=1e-5, atol=1e-7)


def test_uint8_frames_equal_prenormalised_input(hw):
    """SURVEY 8f N4 (first step): raw uint8 RGB frames go straight into the stem pack kernel, which fuses ImageNorm
    (data_utils.py:266-276), the BGR flip and the NHWC pack -- same logits as the fp32 mean-subtracted input."""
    cfg, sd, model = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), torch.float32, hw.dev)
    frames = S.synthetic_frames(2, 2, 64, 13)[..., :64, :].repeat(1, 1, 1, 1, 2).contiguous()        # uint8
    assert frames.dtype == torch.uint8
    ids, mask = S.synthetic_text(2, 6, 13, cfg["vocab_size"])
    ids = ids.clamp(max=cfg["vocab_size"] - 1)
    common = dict(text_input_ids=ids, text_input_mask=mask, labels=None)
    with torch.no_grad():
        a = model(to_dev(dict(common, visual_inputs=frames, n_examples_list=[1, 1]), hw.dev))["logits"]
        b = model(to_dev(dict(common, visual_inputs=O.image_norm(frames, S.PIXEL_MEAN, S.PIXEL_STD), n_examples_list=[1, 1]), hw.dev))["logits"]
    torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6)


def test_pretraining_pixel_random_sampling_train_mode(hw):
    """Pixel-BERT style random sub-sampling of the visual tokens (modeling.py:15-34,80-88): training mode only, indices
    from numpy's global RNG exactly as the reference draws them; forward AND gradients against the oracle."""
    import numpy as np
    extra = dict(pixel_random_sampling_size=1, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg, sd, model = build("pretraining", extra, torch.float32, hw.dev)
    model.train()
    batch = make_batch(cfg, "pretraining", 2, 1, 6)
    mlm = batch["text_input_ids"].clone()
    mlm[:, ::2] = -100
    batch["mlm_labels"] = mlm
    batch["itm_labels"] = S.synthetic_labels(2, 2, 5)
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k) for k, v in sd.items()}
    sdr["transformer.cls.predictions.decoder.weight"] = sdr["transformer.bert.embeddings.word_embeddings.weight"]
    sdr["transformer.cls.predictions.decoder.bias"] = sdr["transformer.cls.predictions.bias"]
    grid = O.grid_feat_backbone(sdr, batch["visual_inputs"], "cnn.")
    lv = grid.shape[2] * grid.shape[3]
    assert lv == 2
    np.random.seed(7)
    idx = torch.from_numpy(np.sort(np.random.choice(lv, size=1, replace=False))).long()
    ref = O.pretraining_forward(sdr, batch["text_input_ids"], grid, batch["text_input_mask"], cfg, mlm, batch["itm_labels"], sample_idx=idx)
    (ref["mlm_loss"].mean() + ref["itm_loss"].mean()).backward()
    np.random.seed(7)                                     # the product draws from the same global RNG
    model.rt.bank.zero_grad()
    out = model(to_dev(dict(batch, n_examples_list=[1, 1]), hw.dev))
    tol = dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)
    torch.testing.assert_close(out["itm_scores"].cpu(), ref["itm_scores"].detach(), **tol)
    torch.testing.assert_close(out["mlm_loss"].cpu(), ref["mlm_loss"].detach(), **tol)
    (out["mlm_loss"].mean() + out["itm_loss"].mean()).backward()
    for name in ("transformer.bert.visual_embeddings.row_position_embeddings.weight", "cnn.grid_encoder.0.weight",
                 "transformer.bert.encoder.layer.0.attention.self.query.weight"):
        p = dict(model.named_parameters())[name]
        g_ref = sdr[name].grad
        diff = (p.grad.cpu() - g_ref).norm() / max(g_ref.norm().item(), 1e-8)
        assert diff < (2e-3 if hw.name == "emul" else 5e-3), (name, float(diff))


@pytest.mark.parametrize("head,extra,repeat,label_kind", [
    ("retrieval", dict(num_labels=1, loss_type="rank", margin=0.1), 2, "unused"),          # a16 ranking loss
    ("multiple_choice", dict(num_labels=5, loss_type="ce"), 5, "per_video"),               # a17 (TGIF-QA action / transition)
    ("sequence_classification", dict(num_labels=7, loss_type="ce"), 1, "class"),           # a18 open-ended QA
    ("sequence_classification", dict(num_labels=6, loss_type="bce"), 1, "soft"),           # a18 VQA-style soft targets
    ("sequence_classification", dict(num_labels=1, loss_type="ce"), 1, "real"),            # a18 regression (count): MSE
])
def test_other_heads_and_losses_match_oracle(hw, head, extra, repeat, label_kind):
    """logits, per-example losses and gradients of the remaining heads / loss types (modeling.py:327-451, 543-580)."""
    cfg, sd, model = build(head, extra, torch.float32, hw.dev)
    n_videos = 2
    batch = make_batch(cfg, head, n_videos, repeat, 6)
    n_pairs = n_videos * repeat
    g = torch.Generator().manual_seed(3)
    if label_kind == "per_video":
        batch["labels"] = torch.randint(0, 5, (n_videos,), generator=g)
    elif label_kind == "class":
        batch["labels"] = torch.randint(0, extra["num_labels"], (n_pairs,), generator=g)
    elif label_kind == "soft":
        batch["labels"] = torch.rand(n_pairs, extra["num_labels"], generator=g)
    elif label_kind == "real":
        batch["labels"] = torch.rand(n_pairs, generator=g) * 10
    else:
        batch["labels"] = torch.zeros(n_pairs, dtype=torch.long)
    ref, sdr = grads_of_oracle(sd, batch, cfg, head, lambda o: o["loss"].mean())
    model.rt.bank.zero_grad()
    out = model(to_dev(batch, hw.dev))
    tol = dict(rtol=1e-3, atol=1e-4) if hw.name == "emul" else dict(rtol=2e-3, atol=1e-3)
    torch.testing.assert_close(out["logits"].cpu(), ref["logits"].detach(), **tol)
    torch.testing.assert_close(out["loss"].cpu().reshape(-1), ref["loss"].detach().reshape(-1), **tol)
    out["loss"].mean().backward()
    params = dict(model.named_parameters())
    # (classifier.2.bias is skipped: for the 1-logit multiple-choice head its gradient is exactly zero, softmax shift invariance)
    for name in ("transformer.classifier.0.weight", "transformer.classifier.2.weight", "transformer.bert.pooler.dense.weight",
                 "transformer.bert.encoder.layer.1.output.dense.weight", "cnn.grid_encoder.0.weight"):
        g_ref = sdr[name].grad
        rel = (params[name].grad.cpu() - g_ref).norm() / max(g_ref.norm().item(), 1e-8)
        assert rel < (2e-3 if hw.name == "emul" else 5e-3), (name, float(rel))


@pytest.mark.parametrize("train_bn", [False, True])
def test_regression_head_matches_oracle(hw, train_bn):
    """ClipBertForRegression (modeling.py:454-507): Linear -> ELU -> BatchNorm1d -> Linear(1), MSE loss; eval mode (running
    statistics) and training mode with the dropouts at 0 (batch statistics + running-estimate update), forward and gradients."""
    extra = dict(num_labels=1, loss_type="mse", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg, sd, model = build("regression", extra, torch.float32, hw.dev)
    model.train(train_bn)
    batch = make_batch(cfg, "regression", 3, 2, 6)
    batch["labels"] = torch.tensor([1.0, 4.0, 2.0, 7.0, 3.0, 5.0])
    out = model(to_dev(dict(batch), hw.dev))
    model.rt.bank.zero_grad()
    out["loss"].mean().backward()
    sdr = {k: v.clone().requires_grad_(v.is_floating_point() and "norm" not in k and "running" not in k) for k, v in sd.items()}
    b2 = dict(batch)
    counts = b2.pop("n_examples_list")
    grid = O.repeat_rows(O.grid_feat_backbone(sdr, b2.pop("visual_inputs"), "cnn."), counts)
    ref = O.regression_forward(sdr, b2["text_input_ids"], grid, b2["text_input_mask"], cfg, labels=b2["labels"], training=train_bn)
    ref["loss"].mean().backward()
    torch.testing.assert_close(out["logits"].float().cpu(), ref["logits"].detach(), rtol=2e-3, atol=2e-4)
    torch.testing.assert_close(out["loss"].float().cpu(), ref["loss"].detach(), rtol=2e-3, atol=2e-3)
    for key in ("transformer.regressor.0.weight", "transformer.regressor.2.weight", "transformer.regressor.2.bias", "transformer.regressor.4.weight",
                "transformer.bert.pooler.dense.weight"):
        p = dict(model.named_parameters())[key]
        g_ref = sdr[key].grad
        scale = max(float(g_ref.abs().max()), 1e-6)
        assert float((p.grad.cpu() - g_ref).abs().max()) / scale < 5e-3, key
    bn = model.transformer.regressor[2]
    if train_bn:                                             # running estimates moved towards the batch statistics, once
        assert int(bn.num_batches_tracked) == 1
        assert float((bn.running_mean.cpu() - sd["transformer.regressor.2.running_mean"]).abs().max()) > 0
    else:
        torch.testing.assert_close(bn.running_var.cpu(), sd["transformer.regressor.2.running_var"], rtol=0, atol=0)


def test_prepare_rejects_overlap_wgrad(hw):
    """the side-stream weight-gradient variants were measured slower and removed: prepare() accepts overlap_wgrad=0 / False only"""
    cfg, _sd, model = build("retrieval", dict(num_labels=2, loss_type="ce", margin=0.1), torch.bfloat16, hw.dev)
    for off in (0, False):
        model.prepare(dtype=torch.bfloat16, device=hw.dev, overlap_wgrad=off)
    for bits in (1, 2, 4, 8, True):
        with pytest.raises(ValueError, match="r06a_overlap_ab"):
            model.prepare(dtype=torch.bfloat16, device=hw.dev, overlap_wgrad=bits)
