"""Masked-LM token masking drawn on the device: cb_mlm_mask / ops.mlm_mask against its NumPy restatement (exact), against the reference's
mask_batch_text_tokens executed from its source (which tokens may be labelled at all), its statistics over the seed words replays would
use, its argument checks, the pretraining loop in ``mlm_masking="device"`` mode against the same loop on batches masked by the
restatement, validate_pretrain, the host logic around it (config, CapturedStep._why_eager, signature, data.mlm_capacity), and -- on the
GPU -- a captured pretraining loop whose replays mask afresh."""
import math
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dropout_restatement as DR
import mlm_mask_restatement as MR
from clipbert_amd import _lib
from clipbert_amd import captured as CAP
from clipbert_amd import config as CFG
from clipbert_amd import data as D
from clipbert_amd import ops, optim, tasks
from clipbert_amd import synthetic as S
from clipbert_amd.modeling import runtime as RT
from oracle import ref_functions, ref_shim
from test_captured_loop import NO_DROP, _assert_same_step, _restore, _result, _small_frames, _snapshot, _text_batch
from test_captured_loop import _tcfg as _cap_tcfg
from test_captured_loop import build_small
from test_mlm_rows import _GridCache, _tcfg, pretrain_batch
from test_model_small import build, make_batch, to_dev

live = pytest.mark.skipif(not ref_shim.available(), reason="reference tree not present")

SENTINEL = -7
V = 30522                                                   # bert-base-uncased
CLS, SEP, PAD, MASK = 101, 102, 0, 103
SHAPES = [(1, 1), (1, 7), (3, 20), (7, 33), (64, 32), (129, 20), (257, 31)]
PROBS = [0.0, 0.15, 0.5, 1.0]
# (host seed, device word or None): no seed_ptr; the model's site at forward 3 under word 5; the wrap-around of the 64-bit sum
SEEDS = [(0, None), (RT._seed(RT._SITE_MLM, 0, 3), 5), ((1 << 64) - 1, 5)]


def _ragged_ids(rows, lt, seed, vocab=V):
    """int64 (rows, lt): [CLS] + tokens of [1000, vocab) + [SEP] + padding, every row its own length (a row of one token is [CLS] alone)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(min(1000, vocab // 2), vocab, (rows, lt), dtype=np.int64)
    n = rng.integers(1, lt + 1, rows)
    ids[:, 0] = CLS
    for r in range(rows):
        if n[r] >= 2:
            ids[r, n[r] - 1] = SEP
        ids[r, n[r]:] = PAD
    return ids


def _launch(hw, ids_np, p, seed, word, inplace=False, odd=False, vocab=V, **kw):
    """-> (ids buffer after, ids_out buffer after, labels buffer after), NumPy, each with its sentinel tail (and, with ``odd``, the ids
    behind one sentinel element: a view that starts 8 bytes into its buffer)"""
    rows, lt = ids_np.shape
    n, off = rows * lt, 1 if odd else 0
    src = torch.full((off + n + 8,), SENTINEL, dtype=torch.int64)
    src[off:off + n] = torch.from_numpy(ids_np.reshape(-1))
    src = src.to(hw.dev)
    ids = src[off:off + n].view(rows, lt)
    assert ids.is_contiguous() and ids.data_ptr() == src.data_ptr() + 8 * off
    out = src if inplace else torch.full((off + n + 8,), SENTINEL, dtype=torch.int64, device=hw.dev)
    lab = torch.full((off + n + 8,), SENTINEL, dtype=torch.int64, device=hw.dev)
    ptr = None if word is None else torch.tensor([word], dtype=torch.int64, device=hw.dev)
    got_ids, got_lab = ops.mlm_mask(ids, p, seed, ptr, vocab_size=vocab, out_ids=out[off:off + n].view(rows, lt),
                                    out_labels=lab[off:off + n].view(rows, lt), **kw)
    assert got_ids.data_ptr() == out.data_ptr() + 8 * off and got_lab.data_ptr() == lab.data_ptr() + 8 * off
    assert got_ids.shape == ids.shape and got_lab.shape == ids.shape
    return src.cpu().numpy(), out.cpu().numpy(), lab.cpu().numpy()


def _check(bufs, ids_np, want, off=0, inplace=False):
    src, out, lab = bufs
    n = ids_np.size
    for name, b in (("ids", src), ("ids_out", out), ("labels", lab)):
        assert (b[:off] == SENTINEL).all() and (b[off + n:] == SENTINEL).all(), (name, b[:off], b[off + n:])
    if not inplace:
        assert np.array_equal(src[off:off + n], ids_np.reshape(-1)), "the input was written"
    assert np.array_equal(out[off:off + n], want[0].reshape(-1))
    assert np.array_equal(lab[off:off + n], want[1].reshape(-1))


# ---- the kernel against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,lt", SHAPES)
def test_kernel_equals_the_restatement(hw, rows, lt):
    ids = _ragged_ids(rows, lt, 100 * rows + lt)
    special = (ids == CLS) | (ids == SEP) | (ids == PAD)
    for p in PROBS:
        for seed, word in SEEDS:
            want = MR.mask(ids, p, DR.effective_seed(seed, word or 0), V)
            _check(_launch(hw, ids, p, seed, word), ids, want)
            labelled = want[1] != -100
            assert not (labelled & special).any() and np.array_equal(want[1][labelled], ids[labelled])
            assert np.array_equal(want[0][~labelled], ids[~labelled])
            if p == 0.0:
                assert not labelled.any() and np.array_equal(want[0], ids)
            if p == 1.0:
                assert np.array_equal(labelled, ~special)


def test_in_place_odd_start_no_specials_no_pad(hw):
    """(7, 33) at p = 0.5 under the model's seed: ids_out is ids; an input (and outputs) that start at an odd element of a larger buffer;
    n_special = 0 ([CLS] / [SEP] are then labelled like words); pad_id = -1 and None (padding is then labelled too)"""
    ids = _ragged_ids(7, 33, 733)
    seed, word = SEEDS[1]
    eff = DR.effective_seed(seed, word)
    plain = MR.mask(ids, 0.5, eff, V)
    _check(_launch(hw, ids, 0.5, seed, word, inplace=True), ids, plain, inplace=True)
    _check(_launch(hw, ids, 0.5, seed, word, odd=True), ids, plain, off=1)
    _check(_launch(hw, ids, 0.5, seed, word, odd=True, inplace=True), ids, plain, off=1, inplace=True)
    bare = MR.mask(ids, 0.5, eff, V, special_ids=())
    _check(_launch(hw, ids, 0.5, seed, word, special_ids=()), ids, bare)
    assert ((bare[1] == CLS) | (bare[1] == SEP)).any() and not (bare[1] == PAD).any()
    nopad = MR.mask(ids, 0.5, eff, V, pad_id=None)
    for pad in (-1, None):
        _check(_launch(hw, ids, 0.5, seed, word, pad_id=pad), ids, nopad)
    assert (nopad[1] == PAD).any() and not np.array_equal(nopad[1], plain[1])
    # other ids in the same roles, the largest vocabulary, a fourth special id
    other = MR.mask(ids, 1.0, eff, 1 << 24, special_ids=(CLS, SEP, 7, int(ids[0, 1])), pad_id=PAD, mask_id=5)
    _check(_launch(hw, ids, 1.0, seed, word, vocab=1 << 24, special_ids=(CLS, SEP, 7, int(ids[0, 1])), mask_id=5), ids, other)
    assert other[1][0, 1] == -100 and (other[0] == 5).any() and other[0].max() > V


def test_allocates_its_outputs(hw):
    ids = torch.from_numpy(_ragged_ids(3, 20, 320)).to(hw.dev)
    before = ids.clone()
    out, lab = ops.mlm_mask(ids, 0.5, 11, vocab_size=V)
    assert out.dtype == lab.dtype == torch.int64 and out.shape == lab.shape == ids.shape and out.device == ids.device
    assert out.data_ptr() != ids.data_ptr() and torch.equal(ids, before)
    want = MR.mask(before.cpu().numpy(), 0.5, 11, V)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(lab.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="vocab_size"):
        ops.mlm_mask(ids, 0.5, 11)


# ---- pinned to the reference ----------------------------------------------------------------------------------------------------------
class _Tokenizer:
    """what mask_batch_text_tokens reads of a BertTokenizer (transformers 2.11.0)"""
    mask_token = "[MASK]"
    _pad_token = "[PAD]"
    pad_token_id = PAD

    def get_special_tokens_mask(self, val, already_has_special_tokens=False):
        assert already_has_special_tokens
        return [1 if x in (CLS, SEP) else 0 for x in val]

    def convert_tokens_to_ids(self, token):
        assert token == "[MASK]"
        return MASK

    def __len__(self):
        return V


@live
def test_which_tokens_can_be_labelled_equals_the_reference(emul):
    """mask_batch_text_tokens at mlm_probability = 1.0 labels exactly the tokens it may ever label ([CLS], [SEP] and padding get
    probability 0, torch.bernoulli(1.0) is 1): its labels equal cb_mlm_mask's at p = 1 element for element, and the replacements of
    both are [MASK], a word of [0, V) or the token itself"""
    fn = ref_functions.load(ref_functions.DATA_UTILS, ["mask_batch_text_tokens"])["mask_batch_text_tokens"]
    ids = _ragged_ids(24, 20, 2420)
    torch.manual_seed(3)
    ref_ids, ref_labels = fn(torch.from_numpy(ids.copy()), _Tokenizer(), mlm_probability=1.0)
    out, lab = ops.mlm_mask(torch.from_numpy(ids.copy()), 1.0, RT._seed(RT._SITE_MLM, 0, 0), vocab_size=V)
    assert torch.equal(lab, ref_labels) and int((lab != -100).sum()) > 100
    assert np.array_equal(lab.numpy(), MR.mask(ids, 1.0, MR.site_seed(0), V)[1])
    for masked in (out.numpy(), ref_ids.numpy()):
        labelled = lab.numpy() != -100
        assert np.array_equal(masked[~labelled], ids[~labelled])
        assert ((masked[labelled] >= 0) & (masked[labelled] < V)).all() and (masked[labelled] == MASK).mean() > 0.6
    # and at probability 0 neither labels anything
    ref_ids0, ref_labels0 = fn(torch.from_numpy(ids.copy()), _Tokenizer(), mlm_probability=0.0)
    out0, lab0 = ops.mlm_mask(torch.from_numpy(ids.copy()), 0.0, 5, vocab_size=V)
    assert torch.equal(lab0, ref_labels0) and torch.equal(out0, ref_ids0) and (lab0 == -100).all()


# ---- statistics -------------------------------------------------------------------------------------------------------------------------
STAT_ROWS, STAT_LT, STAT_SEED, STAT_P, STAT_T = 24, 20, 2420, 0.15, 2000


def _stat_figures(ids, outs, labs, p):
    """-> (sigmas of the labelled share, of the three class shares, of the worst of 16 vocabulary buckets; eligible tokens per draw)"""
    eligible = (ids != CLS) & (ids != SEP) & (ids != PAD)
    labelled = labs != -100
    assert not (labelled & ~eligible[None]).any()
    sig = lambda k, n, q: abs(k - n * q) / math.sqrt(n * q * (1 - q))      # noqa: E731
    n_el, n_lab = int(eligible.sum()) * len(labs), int(labelled.sum())
    is_mask = labelled & (outs == MASK)
    is_kept = labelled & (outs == ids[None])
    is_rand = labelled & ~is_mask & ~is_kept
    words = outs[is_rand]
    share = np.bincount(np.arange(V) * 16 // V, minlength=16) / V          # what a uniform word of [0, V) gives each bucket
    counts = np.bincount(words * 16 // V, minlength=16)
    buckets = max(sig(int(c), words.size, float(q)) for c, q in zip(counts, share))
    return (sig(n_lab, n_el, p), sig(int(is_mask.sum()), n_lab, 0.8), sig(int(is_rand.sum()), n_lab, 0.1), sig(int(is_kept.sum()), n_lab, 0.1),
            buckets, int(eligible.sum()))


def test_statistics_over_the_seed_words_of_replays(hw):
    """A 24 x 20 batch of ragged [CLS] + words + [SEP] + padding rows (_ragged_ids seed 2420: 233 eligible tokens, none of them [MASK]'s id),
    p = 0.15, the model's seed at forward 0, device words 0..1999 -- what 2000 replays of one graph hash with.  Share labelled among
    eligible = p, shares [MASK] / random / kept among labelled = 0.8 / 0.1 / 0.1, the random words uniform over 16 equal vocabulary
    buckets: each within 5 binomial sigma.  (A random word that equals the token it replaces, 1 in V, counts as kept here: some 0.2 events
    in all against a sigma of 80.)  The restatement alone sits at 1.62, 0.20, 0.51, 0.78 sigma and 2.81 sigma for the worst bucket on exactly
    these inputs, and the kernel must equal it."""
    ids = _ragged_ids(STAT_ROWS, STAT_LT, STAT_SEED)
    assert not (ids == MASK).any()
    seed, T = RT._seed(RT._SITE_MLM, 0, 0), STAT_T
    src = torch.from_numpy(ids).to(hw.dev)
    word = torch.zeros(1, dtype=torch.int64, device=hw.dev)
    outs = torch.full((T,) + ids.shape, SENTINEL, dtype=torch.int64, device=hw.dev)
    labs = torch.full((T,) + ids.shape, SENTINEL, dtype=torch.int64, device=hw.dev)
    for t in range(T):
        ops.mlm_mask(src, STAT_P, seed, word, vocab_size=V, out_ids=outs[t], out_labels=labs[t])
        ops.counter_add(word)
    outs, labs = outs.cpu().numpy(), labs.cpu().numpy()                       # the one read-back
    assert int(word.item()) == T
    want = [MR.mask(ids, STAT_P, DR.effective_seed(seed, t), V) for t in range(T)]
    assert np.array_equal(outs, np.stack([w[0] for w in want])) and np.array_equal(labs, np.stack([w[1] for w in want]))
    s_lab, s_mask, s_rand, s_kept, s_bucket, n_el = _stat_figures(ids, outs, labs, STAT_P)
    distinct = len({lab.tobytes() for lab in labs})
    print(f"[mlm_mask statistics] {n_el} eligible: labelled {s_lab:.2f}, [MASK] {s_mask:.2f}, random {s_rand:.2f}, kept {s_kept:.2f}, "
          f"worst bucket {s_bucket:.2f} sigma; {distinct} distinct label patterns of {T}")
    for name, s in (("labelled", s_lab), ("[MASK]", s_mask), ("random", s_rand), ("kept", s_kept), ("bucket", s_bucket)):
        assert s <= 5.0, (name, s)
    assert distinct > 1, "every replay drew the same labels"


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------
def _raw_call(hw, ids=True, out=True, lab=True, rows=3, lt=4, special=(CLS, SEP), n_special=None, vocab=V, p=0.5):
    import ctypes as C
    bufs = [torch.full((32,), SENTINEL, dtype=torch.int64, device=hw.dev) for _ in range(3)]
    bufs[0][:12] = torch.arange(1000, 1012)
    before = [b.clone() for b in bufs]
    arr = (C.c_int64 * 4)(*(list(special) + [0] * (4 - len(special))))
    ptrs = [ops._ptr(b) if use else None for b, use in zip(bufs, (ids, out, lab))]
    rc = _lib.get().cb_mlm_mask(ptrs[0], rows, lt, arr, len(special) if n_special is None else n_special, PAD, MASK, vocab, p, 1, None,
                                ptrs[1], ptrs[2], -100, None)
    if bufs[0].is_cuda:
        torch.cuda.synchronize()
    return rc, all(torch.equal(a, b) for a, b in zip(bufs, before))


@pytest.mark.parametrize("case", [dict(ids=False), dict(out=False), dict(lab=False), dict(rows=0), dict(rows=-1), dict(lt=0), dict(n_special=-1),
                                  dict(n_special=5), dict(vocab=0), dict(vocab=(1 << 24) + 1), dict(p=-0.01), dict(p=1.5), dict(p=float("nan"))],
                         ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_argument_errors_launch_nothing(hw, case):
    rc, untouched = _raw_call(hw, **case)
    assert rc != 0 and untouched
    assert b"cb_mlm_mask" in _lib.get().cb_last_error()
    with pytest.raises(RuntimeError, match="cb_mlm_mask"):
        _lib.check(rc, "cb_mlm_mask")


def test_a_good_call_passes_and_the_abi_names_it(hw):
    rc, untouched = _raw_call(hw)
    assert rc == 0 and not untouched
    assert _raw_call(hw, n_special=0)[0] == 0 and _raw_call(hw, vocab=1 << 24, p=1.0)[0] == 0 and _raw_call(hw, vocab=1, p=0.0)[0] == 0
    assert _lib.get().cb_version() >= 20 and "cb_mlm_mask" in _lib.EXPORTED_SYMBOLS


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
P_LOOP, LT_LOOP = 0.4, 12


class _Spy:
    """records what every ops.mlm_mask call of the loop returned: (ids_out, labels)"""

    def __init__(self, monkeypatch):
        self.calls, real = [], ops.mlm_mask

        def spy(*a, **kw):
            out = real(*a, **kw)
            self.calls.append(out)
            return out

        monkeypatch.setattr(ops, "mlm_mask", spy)


class _Cached(_GridCache):
    """_GridCache with what the task functions read of the model besides its heads"""
    rt = property(lambda self: self.model.rt)
    config = property(lambda self: self.model.config)


_LOOP_MODELS = {}


def _loop_model(hw):
    """-> (cfg, the small fp32 pretraining model without dropout, its grid-caching face): one per backend for the tests below, which all
    show it the frames of _unmasked -- their grid features are computed once.  The tests read the runtime's counters relative to where
    they find them."""
    if hw.name not in _LOOP_MODELS:
        cfg, _sd, inner = build("pretraining", NO_DROP, torch.float32, hw.dev)
        _LOOP_MODELS[hw.name] = (cfg, inner, _Cached(inner), make_batch(cfg, "pretraining", 2, 1, LT_LOOP, 5)["visual_inputs"].to(hw.dev))
    cfg, inner, model, _frames = _LOOP_MODELS[hw.name]
    model.train()
    return cfg, inner, model


def _unmasked(hw, cfg, seed):
    """an unmasked batch on the backend's device: the text of ``seed`` over the one set of frames"""
    batch = to_dev(make_batch(cfg, "pretraining", 2, 1, LT_LOOP, seed), hw.dev)
    batch["visual_inputs"] = _LOOP_MODELS[hw.name][3]
    batch["itm_labels"] = S.synthetic_labels(2, 2, seed).to(hw.dev)
    return batch


def _restated(batch, vocab, fwd_i, word, p=P_LOOP):
    """the batch as a host collator would deliver it, masked by the restatement under (fwd_i, seed word)"""
    ids, lab = MR.site_mask(batch["text_input_ids"].cpu().numpy(), p, fwd_i, word, vocab)
    dev = batch["text_input_ids"].device
    return dict(batch, text_input_ids=torch.from_numpy(ids).to(dev), mlm_labels=torch.from_numpy(lab).to(dev)), lab


def _n_labelled(batch, vocab, fwd_i, word, p=P_LOOP):
    return int((_restated(batch, vocab, fwd_i, word, p)[1] != -100).sum())


def _grads(model):
    return {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad and p.grad is not None}


def test_pretrain_loss_with_device_masking(hw, monkeypatch):
    """tasks.pretrain_loss under mlm_masking = "device" against tasks.pretrain_loss on the batch masked by the restatement under the same
    (forward count, seed word), dropout off: the same kernels on the same inputs, so loss and gradients are equal bit for bit -- except the
    embedding tables, whose gradients the embedding backward adds up through fp32 atomics in whatever order the workgroups arrive (two
    runs of the SAME code differ there in the last bit: tests/test_mlm_rows.py::test_default_mode_is_untouched); those are held to that
    test's bound on one gradient buffer computed twice (rtol 1e-5, atol 1e-7)."""
    cfg, inner, model = _loop_model(hw)
    rt, vocab = inner.rt, cfg["vocab_size"]
    batch = _unmasked(hw, cfg, 5)
    dev_cfg = _tcfg(mlm_rows="labelled", mlm_masking="device", mlm_probability=P_LOOP)
    host_cfg = _tcfg(mlm_rows="labelled")
    fwd0 = rt.forward_count
    # a seed word under which this forward and the next label different positions, both at least one (a condition on the inputs, from
    # the restatement)
    word = next(w for w in range(1, 64) if _n_labelled(batch, vocab, fwd0, w) and _n_labelled(batch, vocab, fwd0 + 1, w)
                and not np.array_equal(_restated(batch, vocab, fwd0, w)[1], _restated(batch, vocab, fwd0 + 1, w)[1]))
    rt.seed_dev.fill_(word)
    spy = _Spy(monkeypatch)
    ids_before = batch["text_input_ids"].clone()

    rt.bank.zero_grad()
    loss = tasks.pretrain_loss(model, dict(batch), dev_cfg)
    loss.backward()
    g_dev = _grads(inner)
    assert rt.forward_count == fwd0 + 1                                   # (dropout is off: the draw alone advances the counter)
    assert len(spy.calls) == 1 and torch.equal(batch["text_input_ids"], ids_before)
    twin, lab = _restated(batch, vocab, fwd0, word)
    assert np.array_equal(spy.calls[0][1].cpu().numpy(), lab) and torch.equal(spy.calls[0][0], twin["text_input_ids"])

    rt.bank.zero_grad()
    loss_h = tasks.pretrain_loss(model, dict(twin), host_cfg)
    loss_h.backward()
    g_host = _grads(inner)
    assert rt.forward_count == fwd0 + 1 and len(spy.calls) == 1           # host mode: no draw, no counter
    assert torch.equal(loss.detach(), loss_h.detach()) and float(loss.detach()) > 0
    assert set(g_dev) == set(g_host) and len(g_dev) > 30
    for name, g in g_dev.items():
        if "embeddings" in name:
            torch.testing.assert_close(g, g_host[name], rtol=1e-5, atol=1e-7)
        else:
            assert torch.equal(g, g_host[name]), name
    assert max(float(g.abs().max()) for g in g_dev.values()) > 0

    # the second step draws other masks: the restatement at the next forward count
    with torch.no_grad():
        loss2 = tasks.pretrain_loss(model, dict(batch), dev_cfg)
        twin2, lab2 = _restated(batch, vocab, fwd0 + 1, word)
        assert rt.forward_count == fwd0 + 2 and len(spy.calls) == 2
        assert np.array_equal(spy.calls[1][1].cpu().numpy(), lab2) and not np.array_equal(lab, lab2)
        assert torch.equal(loss2, tasks.pretrain_loss(model, dict(twin2), host_cfg)) and not torch.equal(loss2, loss.detach())
        assert rt.forward_count == fwd0 + 2

        # evaluation: the batch ordinal is the seed, the seed word is not read, nothing advances
        model.eval()
        for ordinal in (0, 2):
            out = tasks._pretrain_forward(model, dict(batch), dev_cfg, eval_ordinal=ordinal)
            want_ids, want_lab = MR.mask(ids_before.cpu().numpy(), P_LOOP, MR.site_seed(ordinal, 0), vocab)
            assert np.array_equal(out["mlm_labels"].cpu().numpy(), want_lab) and np.array_equal(out["text_input_ids"].cpu().numpy(), want_ids)
            assert out["mlm_scores"] is None and out["mlm_pred"].shape == ids_before.shape
        ev = dict(batch, text_input_ids=torch.from_numpy(MR.mask(ids_before.cpu().numpy(), P_LOOP, MR.site_seed(0, 0), vocab)[0]).to(hw.dev),
                  mlm_labels=torch.from_numpy(MR.mask(ids_before.cpu().numpy(), P_LOOP, MR.site_seed(0, 0), vocab)[1]).to(hw.dev))
        assert torch.equal(tasks.pretrain_loss(model, dict(batch), dev_cfg), tasks.pretrain_loss(model, ev, host_cfg))
        assert rt.forward_count == fwd0 + 2 and int(rt.seed_dev.item()) == word and len(spy.calls) == 5
        # use_mlm off: nothing is drawn, the text goes in as it is
        tasks.pretrain_loss(model, dict(batch), _tcfg(mlm_masking="device", use_mlm=False))
        assert len(spy.calls) == 5

        # a batch that is masked already, and an unknown mode, in training and in evaluation alike
        for training in (False, True):
            model.train(training)
            with pytest.raises(ValueError, match="mlm_labels"):
                tasks.pretrain_loss(model, dict(twin), dev_cfg)
            for cfg_bad in (_tcfg(mlm_masking="gpu"), _tcfg(mlm_masking="gpu", use_mlm=False)):
                with pytest.raises(ValueError, match="mlm_masking"):
                    tasks.pretrain_loss(model, dict(batch), cfg_bad)
                with pytest.raises(ValueError, match="mlm_masking"):
                    tasks.validate_pretrain(model, [dict(twin)], cfg_bad)
        assert rt.forward_count == fwd0 + 2 and len(spy.calls) == 5


def test_host_mode_is_the_default_and_leaves_the_counters_alone(hw, monkeypatch):
    """without the key (and with mlm_masking = "host") the batch's own labels are used as before: cb_mlm_mask is never called and, with
    dropout off, no counter moves"""
    cfg, inner, model = _loop_model(hw)
    batch = _unmasked(hw, cfg, 5)
    batch["mlm_labels"] = pretrain_batch(cfg, lt=LT_LOOP)["mlm_labels"].to(hw.dev)
    spy = _Spy(monkeypatch)
    fwd0, word0 = inner.rt.forward_count, int(inner.rt.seed_dev.item())
    with torch.no_grad():
        a = tasks.pretrain_loss(model, dict(batch), _tcfg(mlm_rows="labelled"))
        b = tasks.pretrain_loss(model, dict(batch), _tcfg(mlm_rows="labelled", mlm_masking="host", mlm_probability=0.9))
        log = tasks.validate_pretrain(model, [dict(batch)], _tcfg(mlm_rows="labelled"))
    assert torch.equal(a, b) and log["valid/mlm_loss"] > 0
    assert not spy.calls and inner.rt.forward_count == fwd0 and int(inner.rt.seed_dev.item()) == word0


def test_validate_pretrain_with_device_masking_repeats_itself(hw, monkeypatch):
    """two passes over the same loader give identical logs, equal to the host-masked validation on the restated masks of ordinals 0, 1, 2
    (no seed word: the runtime's is set to 9 here and must not matter); no counter moves"""
    cfg, inner, model = _loop_model(hw)                                   # (in training mode: validate_pretrain switches to evaluation and back)
    vocab, rt = cfg["vocab_size"], inner.rt
    rt.seed_dev.fill_(9)
    fwd0 = rt.forward_count
    loader = [_unmasked(hw, cfg, s) for s in (5, 6, 7)]
    dev_cfg = _tcfg(mlm_rows="labelled", mlm_masking="device", mlm_probability=P_LOOP)
    spy = _Spy(monkeypatch)
    logs = [tasks.validate_pretrain(model, loader, dev_cfg) for _ in range(2)]
    assert logs[0] == logs[1] and len(spy.calls) == 6 and model.training
    n_tok = 0
    for k in range(3):
        lab = MR.mask(loader[k]["text_input_ids"].cpu().numpy(), P_LOOP, MR.site_seed(k, 0), vocab)[1]
        assert np.array_equal(spy.calls[k][1].cpu().numpy(), lab) and np.array_equal(spy.calls[3 + k][1].cpu().numpy(), lab)
        n_tok += int((lab != -100).sum())
    assert n_tok > 3 and logs[0]["valid/mlm_loss"] > 0
    host = [_restated(b, vocab, k, 0)[0] for k, b in enumerate(loader)]
    assert tasks.validate_pretrain(model, host, _tcfg(mlm_rows="labelled")) == logs[0]
    assert rt.forward_count == fwd0 and int(rt.seed_dev.item()) == 9 and len(spy.calls) == 6


# ---- host logic ---------------------------------------------------------------------------------------------------------------------------
def _stub_model():
    cfg = SimpleNamespace()
    return SimpleNamespace(training=True, config=cfg, transformer=SimpleNamespace(bert=SimpleNamespace(config=cfg)),
                           rt=SimpleNamespace(bank=SimpleNamespace(device=torch.device("cpu"))))


def test_why_eager_and_signature_follow_the_mode():
    plain = dict(visual_inputs=torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8), text_input_ids=torch.zeros(1, 4, dtype=torch.long),
                 text_input_mask=torch.ones(1, 4, dtype=torch.long), itm_labels=torch.zeros(1, dtype=torch.long), n_examples_list=[1])
    masked = dict(plain, mlm_labels=torch.full((1, 4), -100, dtype=torch.long))
    mk = lambda **kw: CAP.CapturedStep(_stub_model(), None, _cap_tcfg(**kw), mode="dry")      # noqa: E731
    reason = "without a fixed mlm_capacity"
    # the labels the batch carries, as before
    assert reason in mk(mlm_rows="labelled")._why_eager(masked) and mk(mlm_rows="labelled", mlm_capacity=64)._why_eager(masked) is None
    assert mk(mlm_rows="labelled")._why_eager(plain) is None and mk(mlm_rows="labelled", mlm_masking="host")._why_eager(plain) is None
    # the labels drawn on the device: the same reason without labels in the batch
    assert reason in mk(mlm_rows="labelled", mlm_masking="device")._why_eager(plain)
    assert reason in mk(mlm_masking="device")._why_eager(plain)                                 # ("labelled" is the default)
    assert mk(mlm_rows="labelled", mlm_masking="device", mlm_capacity=64)._why_eager(plain) is None
    assert mk(mlm_rows="all", mlm_masking="device")._why_eager(plain) is None
    assert mk(mlm_rows="labelled", mlm_masking="device", use_mlm=False)._why_eager(plain) is None
    # the signature
    sig = lambda **kw: mk(mlm_capacity=64, **kw).signature(plain)                               # noqa: E731
    assert sig() == sig(mlm_masking="host") == sig(mlm_masking="host", mlm_probability=0.15)
    assert sig(mlm_masking="device") != sig()
    assert sig(mlm_masking="device", mlm_probability=0.3) != sig(mlm_masking="device")
    assert mk(mlm_capacity=128, mlm_masking="device").signature(plain) != sig(mlm_masking="device")


def test_config_carries_the_keys_and_their_defaults():
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_configs")
    path = os.path.join(root, "src", "configs", "pretrain_image_text_base_resnet50_mlm_itm.json")
    cfg = CFG.load_task_config(path, task="pretraining")
    assert cfg.mlm_masking == "host" and cfg.mlm_probability == 0.15 and cfg.mlm_mask_token_id == 103 and cfg.mlm_special_ids == [101, 102]
    cfg2 = CFG.load_task_config(path, task="pretraining", mlm_masking="device", mlm_probability=0.2)
    assert cfg2.mlm_masking == "device" and cfg2.mlm_probability == 0.2 and cfg2.mlm_special_ids == [101, 102]
    cfg2.mlm_special_ids.append(5)                                        # (a config's list is its own)
    assert CFG.load_task_config(path, task="pretraining").mlm_special_ids == [101, 102]
    assert "mlm_masking" not in CFG.load_task_config(os.path.join(root, "src", "configs", "msrvtt_ret_base_resnet50.json"))
    assert tasks._mlm_masking(cfg) == "host" and tasks._mlm_masking(cfg2) == "device" and tasks._mlm_masking(SimpleNamespace()) == "host"


def test_mlm_capacity():
    """min(rows, ceil(rows p + sigmas sqrt(rows p (1 - p)))) rounded up to 64: by hand for a few (rows, p); a multiple of 64; never above
    ``rows`` (rounded up to 64 where rows itself is no multiple: the head rounds its slots to 64 anyway)"""
    # 1280 x 0.15 = 192, sigma = sqrt(163.2) = 12.77: 192 + 76.6 -> 269 -> 320
    assert D.mlm_capacity(1280) == 320 and D.mlm_capacity(1280, 0.15, 6.0) == 320
    assert D.mlm_capacity(1280, sigmas=0.0) == 192                        # the mean itself
    assert D.mlm_capacity(640, 0.15) == 192                               # 96 + 6 x 9.03 = 150.2 -> 151 -> 192
    assert D.mlm_capacity(64, 0.5) == 64                                  # 32 + 24 = 56 -> 64
    assert D.mlm_capacity(12, 0.15) == 64 and D.mlm_capacity(1, 1.0) == 64
    assert D.mlm_capacity(1280, 1.0) == 1280 and D.mlm_capacity(1280, 0.0) == 64 and D.mlm_capacity(1280, 0.9) == 1280
    for rows in (1, 24, 64, 100, 480, 640, 1280, 4096, 65536):
        for p in (0.0, 0.05, 0.15, 0.5, 0.97, 1.0):
            cap = D.mlm_capacity(rows, p)
            assert cap % 64 == 0 and 64 <= cap <= (rows + 63) // 64 * 64, (rows, p, cap)
            if rows % 64 == 0:
                assert cap <= rows
            assert cap >= min(rows, rows * p)
    for bad in (dict(rows=0), dict(rows=5, p=1.5), dict(rows=5, p=-0.1), dict(rows=5, sigmas=-1.0)):
        with pytest.raises(ValueError):
            D.mlm_capacity(**bad)


# ---- captured pretraining with the masks drawn inside the step ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_pretraining_with_device_masking_is_captured_and_masks_afresh(monkeypatch):
    dev = torch.device("cuda", 0)
    cfg, _sd, model = build_small("pretraining", NO_DROP, torch.bfloat16, dev)
    model.train(True)
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=5.0)
    rt, vocab = model.rt, cfg["vocab_size"]
    batches = []
    for i in range(5):
        b = _text_batch(_small_frames(90 + i, dev=dev), 1, LT_LOOP, 90 + i, vocab, dev)
        del b["labels"]
        batches.append(dict(b, itm_labels=torch.tensor([1, 0]).to(dev)))
    common = dict(train_n_clips=1, num_frm=2, mlm_rows="labelled", mlm_capacity=64)
    tcfg = _cap_tcfg(mlm_masking="device", mlm_probability=P_LOOP, **common)
    host_cfg = _cap_tcfg(**common)
    loss_fn = tasks.pretrain_loss
    # eager steps leave the seed word alone, every replay adds one: the three replays hash with fwd_cap and w0, w0 + 1, w0 + 2.  fwd_cap is
    # the counter the capture (second sight) sees: one eager forward after now.  w0: the first word under which the three replays label
    # at least one token each and consecutive ones label different positions (a condition on the inputs, from the restatement).
    fwd_cap = rt.forward_count + 1

    def labels_of(k, w):
        return _restated(batches[k], vocab, fwd_cap, w)[1]

    w0 = next(w for w in range(64) if all((labels_of(2 + j, w + j) != -100).any() for j in range(3))
              and all(not np.array_equal(labels_of(2 + j, w + j) != -100, labels_of(3 + j, w + j + 1) != -100) for j in range(2)))
    rt.seed_dev.fill_(w0)
    spy = _Spy(monkeypatch)
    stepper = CAP.CapturedStep(model, opt, tcfg, loss_fn=loss_fn)
    graph_out = {}

    def run_captured(b, k):
        before = len(spy.calls)
        loss = stepper.step(b, k)
        torch.cuda.synchronize()
        if k == 1:                                                           # the capture's own call comes first: its outputs are the graph's
            graph_out["ids"], graph_out["labels"] = spy.calls[before]
        if k >= 2:                                                           # (a replay calls nothing)
            assert len(spy.calls) == before
        return loss

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for k, b in enumerate(batches):
            replay = k >= 2
            fwd_before, word_before = rt.forward_count, int(rt.seed_dev.item())
            snap = _snapshot(model, opt)
            got = _result(model, opt, run_captured(b, k))
            word_after = int(rt.seed_dev.item())
            if k == 1:
                assert fwd_before == fwd_cap
            if replay:
                assert word_after == word_before + 1 and word_before == w0 + (k - 2) and rt.forward_count == fwd_before
                # what the graph drew and counted: the restatement for (fwd_cap, the word it hashed with)
                twin, lab = _restated(b, vocab, fwd_cap, word_before)
                assert np.array_equal(graph_out["labels"].cpu().numpy(), lab) and torch.equal(graph_out["ids"], twin["text_input_ids"])
                assert model.transformer.mlm_counts.cpu().tolist() == [int((lab != -100).sum()), 0]
                # the host-masked step on the restated batch, from the same weights
                _restore(model, opt, snap)
                want_host = _result(model, opt, tasks.train_step(model, opt, twin, host_cfg, k, loss_fn=loss_fn))
                _assert_same_step(model, got, want_host, f"device-masked replay {k} against the restated host-masked step")
            # the eager twin: the graph's host half of the seed is frozen at the capture's count
            _restore(model, opt, snap)
            if replay:
                rt.forward_count = fwd_cap
            want = _result(model, opt, tasks.train_step(model, opt, b, tcfg, k, loss_fn=loss_fn))
            _assert_same_step(model, got, want, f"device-masked pretraining step {k}")
            if replay:
                rt.forward_count = fwd_before                                # (the twin counted from fwd_cap)
                rt.seed_dev.fill_(word_after)                                # and the word goes on from where the replay left it
    assert not [w for w in caught if "runs eagerly" in str(w.message)], [str(w.message) for w in caught]
    assert stepper.log == ["eager", "eager", "replay", "replay", "replay"], stepper.log
    assert stepper.stats["fallbacks"] == 0 and stepper.stats["captures"] == 1, stepper.stats
    assert int(rt.seed_dev.item()) == w0 + 3
