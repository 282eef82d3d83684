"""Round 6: the squared gradient norm of a single-process step comes from the shares the weight-gradient launches leave behind
(cb_gemm_desc.sq_slots -> ParamBank.fold_* -> cb_sq_sum_fold) instead of a second pass over the gradients, and the ResNet's convolution
weight gradients are STORED by their first writer (accumulate = 2) instead of accumulated into a zero-filled range.  Same step, both
ways, on the host emulator and the GPU: the same norm up to the order of fp32 additions, the same update; a second backward of the step
(gradient accumulation) voids the shares and the full pass runs; a gradient exchange blocks them."""
from types import SimpleNamespace

import pytest
import torch

from clipbert_amd import optim, tasks
from clipbert_amd import synthetic as S
from oracle import clipbert_oracle as O
from test_model_small import build, to_dev

RET = dict(num_labels=2, loss_type="ce", margin=0.1)
TCFG = SimpleNamespace(train_n_clips=2, num_frm=2, score_agg_func="lse", learning_rate=1e-3, cnn_learning_rate=1e-3, decay="linear",
                       cnn_lr_decay="linear", num_train_steps=10, warmup_ratio=0.1, gradient_accumulation_steps=1)


def _batch(dev, cfg, seed=5):
    f = S.synthetic_frames(2, 4, 64, seed)
    vis = O.image_norm(f, S.PIXEL_MEAN, S.PIXEL_STD)
    ids, mask = S.synthetic_text(4, 6, seed, cfg["vocab_size"])
    return to_dev(dict(visual_inputs=vis, text_input_ids=ids.clamp(max=cfg["vocab_size"] - 1), text_input_mask=mask, labels=torch.tensor([1, 0, 1, 0]),
                       n_examples_list=[2, 2]), dev)


def _one_step(hw, monkeypatch, fold, acc_steps=1, block=False):
    cfg, sd, model = build("retrieval", RET, torch.bfloat16, hw.dev)
    model.eval()                                                   # (dropout off: both arms see the same forward)
    bank = model.rt.bank
    opt = optim.FusedAdamW(bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=0.05, fold_norm=fold)
    if block:
        bank.block_norm_fold()
    tcfg = SimpleNamespace(**dict(vars(TCFG), gradient_accumulation_steps=acc_steps))
    used = []
    real = bank.fold_result
    monkeypatch.setattr(bank, "fold_result", lambda: used.append(real()) or used[-1])
    for micro in range(acc_steps):
        tasks.train_step(model, opt, dict(_batch(hw.dev, cfg)), tcfg, global_step=0, micro_step=micro)
    norm2 = float(opt._sq.float().cpu())
    return norm2, bank.grad[:bank.n_train].clone().cpu(), bank.master[:bank.n_train].clone().cpu(), used, bank


def test_folded_norm_and_first_writer_stores_equal_the_full_pass(hw, monkeypatch):
    n_fold, g_fold, p_fold, used, bank = _one_step(hw, monkeypatch, True)
    n_full, g_full, p_full, used0, _ = _one_step(hw, monkeypatch, False)
    assert used and used[-1] is not None and not used0             # the shares were used / never consulted
    segs, slots = used[-1]
    covered = bank.n_train - sum(hi - lo for lo, hi in segs)
    assert covered > 0.5 * bank.n_train                            # encoder + ResNet weights: most of the gradient never re-read
    assert covered == (bank.lazy_span[1] - bank.lazy_span[0]) + (bank.fresh_span[1] - bank.fresh_span[0])
    assert torch.isfinite(g_fold).all()
    for a, b in (bank.lazy_span, bank.fresh_span):               # first-writer stores: the same weight gradients bit for bit (ordered slab sums)
        torch.testing.assert_close(g_fold[a:b], g_full[a:b], rtol=0, atol=0)
    torch.testing.assert_close(g_fold, g_full, rtol=1e-5, atol=1e-9)      # (embedding scatters add through atomics: order of arrival)
    assert abs(n_fold - n_full) <= 2e-6 * n_full, (n_fold, n_full)
    assert n_full > 0.05 ** 2                                      # (the clip is active: the norm matters)
    torch.testing.assert_close(p_fold, p_full, rtol=1e-5, atol=1e-7)
    want = float((g_full.double() ** 2).sum())
    assert abs(n_fold - want) <= 1e-5 * want


def test_gradient_accumulation_and_exchanges_fall_back_to_the_full_pass(hw, monkeypatch):
    n2, g2, _p, used, _ = _one_step(hw, monkeypatch, True, acc_steps=2)
    assert used and used[-1] is None                               # a second backward accumulated: the first one's shares are void
    want = float((g2.double() ** 2).sum())
    assert abs(n2 - want) <= 1e-5 * want
    n1, g1, _p, used, _ = _one_step(hw, monkeypatch, True, block=True)     # (what GradSync does when there is something to exchange)
    assert used and used[-1] is None
    want = float((g1.double() ** 2).sum())
    assert abs(n1 - want) <= 1e-5 * want



def _prepared(hw, fold=True):
    cfg, _sd, model = build("retrieval", RET, torch.bfloat16, hw.dev)
    model.eval()                                                   # (dropout off)
    opt = optim.FusedAdamW(model.rt.bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=0.05, fold_norm=fold)
    return cfg, model, model.rt.bank, opt


def test_grad_norm_survives_the_next_lazy_zero_grad(hw, monkeypatch):
    """the folded norm is STORED into the optimizer's own word (cb_sq_sum_fold: out =), not into the slot buffer that the next
    zero_grad(lazy=True) clears: grad_norm() still reports the step that ran, and a deferred launch(prev=True, reuse_norm=True) clips with it"""
    cfg, model, bank, opt = _prepared(hw)
    used = []
    real = bank.fold_result
    monkeypatch.setattr(bank, "fold_result", lambda: used.append(real()) or used[-1])
    tasks.train_step(model, opt, dict(_batch(hw.dev, cfg)), TCFG, global_step=0)
    assert used and used[-1] is not None                           # the norm came from the shares
    norm = opt.grad_norm()
    assert norm > 0.05                                             # (the clip is active)
    opt.zero_grad(lazy=True)
    assert opt.grad_norm() == norm


def test_partial_backward_exchanges_zeros_for_unwritten_first_writer_gradients(hw):
    """after zero_grad(lazy=True) the ResNet's weight-gradient range is not zeroed: its first writers store.  A backward that never reaches
    the ResNet leaves it unwritten; what GradSync casts onto the wire (dry world 2: every step of a rank but the collectives) is zeros there,
    not what the buffer held before."""
    from clipbert_amd.dist import GradSync
    cfg, model, bank, opt = _prepared(hw)
    sync = GradSync(bank, compress="bf16", pretend_world=2)
    assert sync.active and sync.dry
    b = _batch(hw.dev, cfg)
    opt.zero_grad(lazy=True)
    a, e = bank.fresh_span
    bank.grad[a:e].fill_(float("nan"))                            # (garbage made visible)
    with torch.no_grad():
        grid = model.grid_features(b["visual_inputs"])           # no ResNet backward: no convolution weight gradient is written
    b["visual_inputs"] = grid
    model.forward_from_grid(b)["loss"].mean().backward()
    sync.reduce_transformer()
    sync.reduce_cnn()
    sync.wait(cast_back=False)
    wire = sync.wire_gradients()
    assert torch.isfinite(wire.float()).all()
    assert float(wire[a:e].float().abs().max()) == 0.0
    assert float(bank.grad[a:e].abs().max()) == 0.0
    lo, hi = bank.lazy_span
    assert float(wire[lo:hi].float().abs().max()) > 0              # (the encoder's weight gradients did travel)


def test_full_backward_needs_no_finishing_launch(hw, monkeypatch):
    """every reader of the gradients calls ParamBank.finish over its range; after a full backward every first writer has stored, so
    finish launches nothing -- in the one-graph step bench.py captures and in the data-parallel step (dry world 2, hooks armed:
    grid_encoder + res5 leave from the res5 point of the ResNet backward)"""
    from clipbert_amd.bench import step as bench_step
    from clipbert_amd.dist import GradSync
    for dp in (False, True):
        cfg, model, bank, opt = _prepared(hw)
        b = _batch(hw.dev, cfg)
        sync = GradSync(bank, compress="bf16", pretend_world=2 if dp else 0)
        if dp:
            sync.attach(model)
            assert sync.c_early                                     # (the early exchange of grid_encoder + res5 is armed)
        fns = bench_step.make_step(model, b, TCFG, opt, sync, b["labels"], b["n_examples_list"], TCFG.train_n_clips, TCFG.num_frm,
                                   TCFG.score_agg_func)
        calls = []
        real = bank.finish
        monkeypatch.setattr(bank, "finish", lambda lo, hi, **kw: calls.append((lo, hi, real(lo, hi, **kw))) or calls[-1][2])
        fns.host_prepare()
        if not dp:
            fns.device_step()                                       # bench.py's one-GPU step
            assert calls == [(0, bank.n_train, 0)]
            continue
        opt.zero_grad(lazy=True)                                    # bench.py's data-parallel step (device_step_dp)
        fns.forward_loss().backward(fns.one)
        sync.reduce_cnn()
        g16 = sync.wire_gradients()
        sync.wait(cast_back=False)
        opt.launch(grad16=g16)
        assert calls and all(n == 0 for _lo, _hi, n in calls), calls
        # in this order: the transformer range (end of the encoder backward), grid_encoder + res5 (the res5 point of the ResNet backward),
        # the rest of the CNN range, the whole buffer (FusedAdamW.launch); a range again per bucket cast
        assert list(dict.fromkeys((lo, hi) for lo, hi, _n in calls)) == [sync.t_range] + sync.c_early + sync._cnn_late() + [(0, bank.n_train)]
        assert sync.late_ranges == 0
