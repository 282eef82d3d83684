"""cfg.optim = "adam" / "adamax": cb_optim_step's two kernels against the installed torch.optim.Adam / torch.optim.Adamax on CPU in
fp32 -- the very classes the reference's setup_e2e_optimizer instantiates (src/optimization/utils.py:118-127) --, FusedAdam / FusedAdamax
on the parameter bank in every launch mode, and the config / checkpoint surface.  Each case runs on the host emulator build and, marked
`gpu`, on the MI355X.

Bounds are those of test_kernels_misc.test_adamw_matches_reference_restatement_with_clipping: p rtol 1e-6 / atol 1e-7, exp_avg rtol 1e-5 /
atol 1e-7, second state rtol 1e-5 / atol 1e-8.  The kernels form 1 - beta in fp32 (1 - 0.98f is 9.5e-7 off 0.02, 1 - 0.9f 3.6e-7 off 0.1)
where torch rounds the double once, and torch writes exp_avg as a lerp: both far inside 1e-5; on p they are scaled by lr."""
import json
from types import SimpleNamespace

import pytest
import torch

from clipbert_amd import _lib, ops, optim, tasks
from clipbert_amd import config as C
from clipbert_amd._lib import HP_SKIP, OPT_ADAM, OPT_ADAMAX, OPT_ADAMW
from test_model_small import build
from test_norm_fold import RET, TCFG, _batch

P_TOL, M_TOL, V_TOL = dict(rtol=1e-6, atol=1e-7), dict(rtol=1e-5, atol=1e-7), dict(rtol=1e-5, atol=1e-8)
ALGOS = [("adam", OPT_ADAM), ("adamax", OPT_ADAMAX)]
TORCH_CLS = dict(adam=torch.optim.Adam, adamax=torch.optim.Adamax)
OURS = dict(adam=optim.FusedAdam, adamax=optim.FusedAdamax, adamw=optim.FusedAdamW)
SECOND = dict(adam="exp_avg_sq", adamax="exp_inf")
LR, BETAS, EPS, MAX_NORM = 5e-5, (0.9, 0.98), 1e-8, 5.0
G_SEED = 47            # gradients _rnd(n, G_SEED + step, 3.0): their norm exceeds MAX_NORM in all three steps at n = 3 too (7.1, 7.4, 8.5)


def _rnd(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


_TORCH_RUNS = {}


def _torch_three_steps(algo, n, wd):
    """p, exp_avg, second state of the torch class after clip_grad_norm_ + step() on three fresh gradients (computed once per case)"""
    key = (algo, n, wd)
    if key not in _TORCH_RUNS:
        p = torch.nn.Parameter(_rnd(n, 1))
        opt = TORCH_CLS[algo]([p], lr=LR, betas=BETAS, weight_decay=wd)
        for s in range(3):
            p.grad = _rnd(n, G_SEED + s, 3.0)
            total = torch.nn.utils.clip_grad_norm_([p], MAX_NORM)
            assert float(total) > MAX_NORM                                   # the clip is active in every step
            opt.step()
        st = opt.state[p]
        _TORCH_RUNS[key] = (p.detach().clone(), st["exp_avg"].clone(), st[SECOND[algo]].clone())
    return _TORCH_RUNS[key]


def _three_steps(hw, code, n, wd, g16=False, eps=EPS, state=None):
    """the same three steps through cb_optim_step from zero moments (``state``: buffers to update in place instead of fresh ones)"""
    if state is None:
        state = [hw(_rnd(n, 1)), torch.zeros(n, device=hw.dev), torch.zeros(n, device=hw.dev), torch.zeros(n, dtype=torch.bfloat16, device=hw.dev)]
    p, m, v, w16 = state
    ws = torch.zeros(1024, device=hw.dev)
    for s in range(3):
        g = hw(_rnd(n, G_SEED + s, 3.0))
        if g16 is not False:
            g = g.bfloat16() if g16 == "bf16" else g.bfloat16().float()     # bf16 gradients / fp32 gradients holding the same values
        sq = torch.zeros(1, device=hw.dev)
        ops.sq_sum(g, sq, ws)
        hp = torch.tensor(ops.adamw_hyper(LR, BETAS[0], BETAS[1], eps, wd, s + 1, max_norm=MAX_NORM), device=hw.dev)
        ops.optim_step(code, p, g, m, v, w16, hp, sq)
    return p, m, v, w16


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("n", [1003, 3])                                     # vector body + 3-element tail / the tail alone
@pytest.mark.parametrize("algo,code", ALGOS)
def test_kernel_matches_torch_over_three_steps(hw, algo, code, n, wd):
    pr, mr, vr = _torch_three_steps(algo, n, wd)
    p, m, v, w16 = _three_steps(hw, code, n, wd)
    for name, got, want in (("p", p, pr), ("exp_avg", m, mr), (SECOND[algo], v, vr)):
        d = (got.cpu() - want).abs()
        print(f"{algo} n={n} wd={wd} {name}: max abs diff {float(d.max()):.3e}, max rel diff {float((d / want.abs().clamp_min(1e-30)).max()):.3e}")
    torch.testing.assert_close(p.cpu(), pr, **P_TOL)
    torch.testing.assert_close(m.cpu(), mr, **M_TOL)
    torch.testing.assert_close(v.cpu(), vr, **V_TOL)
    assert torch.equal(w16, p.bfloat16())


@pytest.mark.parametrize("algo,code", ALGOS)
def test_bf16_gradients_equal_fp32_gradients_of_the_same_values(hw, algo, code):
    a = _three_steps(hw, code, 1003, 1e-3, g16="bf16")
    b = _three_steps(hw, code, 1003, 1e-3, g16="as_f32")
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("g16", [False, "bf16"])
def test_adamw_through_optim_step_is_cb_adamw(hw, g16):
    n = 1003
    got = _three_steps(hw, OPT_ADAMW, n, 1e-3, g16=g16, eps=1e-6)
    p, m, v, w16 = hw(_rnd(n, 1)), torch.zeros(n, device=hw.dev), torch.zeros(n, device=hw.dev), torch.zeros(n, dtype=torch.bfloat16, device=hw.dev)
    ws = torch.zeros(1024, device=hw.dev)
    for s in range(3):
        g = hw(_rnd(n, G_SEED + s, 3.0))
        g = g.bfloat16() if g16 else g
        sq = torch.zeros(1, device=hw.dev)
        ops.sq_sum(g, sq, ws)
        ops.adamw(p, g, m, v, w16, torch.tensor(ops.adamw_hyper(LR, BETAS[0], BETAS[1], 1e-6, 1e-3, s + 1, max_norm=MAX_NORM), device=hw.dev), sq)
    for x, y in zip(got, (p, m, v, w16)):
        assert torch.equal(x, y)


@pytest.mark.parametrize("algo,code", ALGOS)
def test_skip_flag_and_sliced_buffers(hw, algo, code):
    n = 1003
    p, g, m, v = hw(_rnd(n, 1)), hw(_rnd(n, G_SEED, 3.0)), hw(_rnd(n, 3, 0.1)), hw(_rnd(n, 4).abs() * 0.01)
    w16 = torch.full((n,), 7.0, dtype=torch.bfloat16, device=hw.dev)
    hp = torch.tensor(ops.adamw_hyper(LR, BETAS[0], BETAS[1], EPS, 1e-3, 1, max_norm=MAX_NORM), device=hw.dev)
    hp[HP_SKIP] = 1.0
    before = [t.clone() for t in (p, m, v, w16)]
    ops.optim_step(code, p, g, m, v, w16, hp, torch.tensor([9.0], device=hw.dev))
    for x, y in zip((p, m, v, w16), before):
        assert torch.equal(x, y)                                             # a non-zero CB_HP_SKIP: nothing is written
    # views that start at element 4 of larger buffers: the same result as fresh tensors, nothing outside the views written
    fresh = _three_steps(hw, code, n, 1e-3)
    big = [torch.full((n + 8,), 5.0, dtype=dt, device=hw.dev) for dt in (torch.float32, torch.float32, torch.float32, torch.bfloat16)]
    views = [b[4:4 + n] for b in big]
    views[0].copy_(hw(_rnd(n, 1)))
    views[1].zero_()
    views[2].zero_()
    _three_steps(hw, code, n, 1e-3, state=views)
    for b, f in zip(big, fresh):
        assert torch.equal(b[4:4 + n], f)
        assert float((b[:4].float() - 5.0).abs().max()) == 0.0 and float((b[4 + n:].float() - 5.0).abs().max()) == 0.0


def test_bad_arguments_fail_with_a_message_and_launch_nothing(hw):
    n = 16
    p, g, m, v = (hw(_rnd(n, i)) for i in range(4))
    hp = torch.tensor(ops.adamw_hyper(LR, BETAS[0], BETAS[1], EPS, 0.0, 1), device=hw.dev)
    before = [t.clone() for t in (p, m, v)]
    with pytest.raises(RuntimeError, match="unknown algo 7"):
        ops.optim_step(7, p, g, m, v, None, hp, None)
    lib, ptr = _lib.get(), ops._ptr
    assert lib.cb_optim_step(OPT_ADAM, 5, ptr(p), ptr(g), ptr(m), ptr(v), None, n, ptr(hp), None, None) != 0
    assert b"grad_dtype" in lib.cb_last_error()
    for i in range(5):                                                       # a null p / g / m / v2 / hyper
        args = [ptr(p), ptr(g), ptr(m), ptr(v), None, n, ptr(hp)]
        args[i if i < 4 else 6] = None
        assert lib.cb_optim_step(OPT_ADAMAX, _lib.CB_F32, *args, None, None) != 0
        assert b"null pointer" in lib.cb_last_error()
    if hw.name == "gpu":
        torch.cuda.synchronize()
    for x, y in zip((p, m, v), before):
        assert torch.equal(x, y)


# ---- the optimizer on the bank (the tiny model of test_model_small) -----------------------------------------------------------------
# Adam and Adamax put the weight decay on the gradient: g_eff = c g + wd p.  Among the 26 M parameters of the tiny model a few hundred have
# c g within 1e-7 of -wd p (both are ~1e-5), and where |g_eff| falls below eps = 1e-8 the first step's update lr g_eff / (|g_eff| + eps) moves
# by lr * d / eps for an error d of g_eff.  Two things follow for a comparison at atol 1e-7:
#  - the clip coefficient c has to be the same on both sides to fp32 rounding.  torch.nn.utils.clip_grad_norm_ on CPU is not that exact: over
#    these gradients its fp32 norm is 2.6e-5 (relative) below the float64 norm, the library's 1e-8 -- so the torch side clips with the float64
#    norm of the gradients (the truth test_norm_fold measures the library's norm against, too) and then runs the torch class's step();
#  - an fp32 rounding of c g or wd p (d <= 6e-8 * 1e-4) costs up to lr * 6e-4: the steps run at the reference's learning rate 5e-5 (3e-8),
#    not at the 1e-3 of test_norm_fold's TCFG (6e-7).
BANK_LR = 5e-5
BANK_CLIP = 0.01       # (the gradient norms of the two batches are 0.051 and 0.031 in fp32, 0.015 in the second bf16 step: always clipped)
BANK_TCFG = SimpleNamespace(**dict(vars(TCFG), learning_rate=BANK_LR, cnn_learning_rate=BANK_LR))
BANK_KW = dict(lr=BANK_LR, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=BANK_LR, max_grad_norm=BANK_CLIP)


def _clip_like_torch(params, max_norm):
    """clip_grad_norm_'s arithmetic (coef = max_norm / (total + 1e-6), clamped to 1, grads scaled in place) on the float64 norm"""
    total = float(sum(p.grad.double().pow(2).sum() for p in params).sqrt())
    coef = torch.clamp(torch.tensor(max_norm / (total + 1e-6), dtype=torch.float32), max=1.0)
    for p in params:
        p.grad.mul_(coef)
    return total


def _bank_state(bank):
    return [t.clone() for t in (bank.master, bank.exp_avg, bank.exp_avg_sq)] + ([bank.w16.clone()] if bank.w16 is not None else [])


def _restore(bank, state):
    for t, s in zip((bank.master, bank.exp_avg, bank.exp_avg_sq, bank.w16), state):
        t.copy_(s)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("algo", ["adam", "adamax"])
def test_train_steps_match_torch_on_the_eight_groups(hw, algo, dtype):
    """two tasks.train_step's; the gradients each left in bank.grad replayed through the torch class over the optimizer's eight ranges as
    eight flat tensors (the torch parameters restart from the bank's pre-step masters, the torch moments carry over)"""
    cfg, _sd, model = build("retrieval", RET, dtype, hw.dev)
    model.eval()                                                             # (dropout off)
    bank = model.rt.bank
    opt = OURS[algo](bank, **BANK_KW)
    assert opt.eps == 1e-8
    ranges = [pg["range"] for pg in opt.param_groups]
    assert len(ranges) == 8 and sum(b > a for a, b in ranges) >= 4 and sum(b - a for a, b in ranges) == bank.n_train
    assert {pg["weight_decay"] for pg in opt.param_groups if pg["range"][1] > pg["range"][0]} == {0.0, 1e-3}
    params = [torch.nn.Parameter(torch.zeros(b - a)) for a, b in ranges]
    ref = TORCH_CLS[algo]([dict(params=[p], weight_decay=pg["weight_decay"]) for p, pg in zip(params, opt.param_groups)], lr=BANK_LR, betas=(0.9, 0.98))
    for step in range(2):
        before = bank.master[:bank.n_train].clone().cpu()
        tasks.train_step(model, opt, dict(_batch(hw.dev, cfg, seed=5 + step)), BANK_TCFG, global_step=step)
        grad = bank.grad[:bank.n_train].clone().cpu()
        for p, (a, b), pg, tg in zip(params, ranges, opt.param_groups, ref.param_groups):
            p.data.copy_(before[a:b])
            p.grad = grad[a:b].clone()
            tg["lr"] = pg["lr"]                                              # (the schedule train_step applied)
        total = _clip_like_torch(params, BANK_CLIP)
        assert total > BANK_CLIP                                                  # the clip is active
        assert abs(opt.grad_norm() - total) <= 1e-6 * total
        ref.step()
        after = bank.master[:bank.n_train].cpu()
        want = before.clone()
        for p, (a, b) in zip(params, ranges):
            want[a:b] = p.detach()
        d = (after - want).abs()
        print(f"{algo} {dtype} step {step + 1}: masters max abs diff {float(d.max()):.3e}; moved by up to {float((after - before).abs().max()):.3e}")
        assert float((after - before).abs().max()) > 0.5 * BANK_LR
        torch.testing.assert_close(after, want, **P_TOL)
        if dtype == torch.bfloat16:
            assert torch.equal(bank.w16[:bank.n_train], bank.master[:bank.n_train].bfloat16())
    for p, (a, b) in zip(params, ranges):
        if b == a:
            continue
        torch.testing.assert_close(bank.exp_avg[a:b].cpu(), ref.state[p]["exp_avg"], **M_TOL)
        torch.testing.assert_close(bank.exp_avg_sq[a:b].cpu(), ref.state[p][SECOND[algo]], **V_TOL)


@pytest.mark.parametrize("algo", ["adam", "adamax"])
def test_folded_norm_equals_the_full_pass(hw, algo):
    """fold_norm=True (bf16): the norm from the shares the weight-gradient launches left; then, from the same start and over the SAME
    gradients, a step that takes the full pass: the same masters within what test_norm_fold allows FusedAdamW (rtol 1e-5 / atol 1e-7; the
    clip coefficient differs by the order of fp32 additions)"""
    cfg, _sd, model = build("retrieval", RET, torch.bfloat16, hw.dev)
    model.eval()
    bank = model.rt.bank
    fold, full = OURS[algo](bank, **BANK_KW, fold_norm=True), OURS[algo](bank, **BANK_KW, fold_norm=False)
    assert fold.fold_norm and not full.fold_norm
    start = _bank_state(bank)
    used = []
    real = bank.fold_result
    bank.fold_result = lambda: used.append(real()) or used[-1]
    tasks.train_step(model, fold, dict(_batch(hw.dev, cfg)), BANK_TCFG, global_step=0)
    assert used and used[-1] is not None                                     # the shares were used
    p_fold, n_fold = bank.master[:bank.n_train].clone().cpu(), float(fold._sq.cpu())
    _restore(bank, start)
    for pg, src in zip(full.param_groups, fold.param_groups):
        pg["lr"] = src["lr"]                                                 # (the schedule train_step applied)
    del used[:]
    full.step()                                                              # bank.grad still holds the step's gradients
    assert not used                                                          # ... never consulted
    p_full, n_full = bank.master[:bank.n_train].cpu(), float(full._sq.cpu())
    print(f"{algo}: squared norm folded {n_fold!r}, full pass {n_full!r}; masters differ by up to {float((p_fold - p_full).abs().max()):.3e}")
    assert n_full > BANK_CLIP ** 2 and abs(n_fold - n_full) <= 2e-6 * n_full       # (the clip is active: the norm matters)
    assert float((p_full - start[0][:bank.n_train].cpu()).abs().max()) > 0.5 * BANK_LR
    torch.testing.assert_close(p_fold, p_full, rtol=1e-5, atol=1e-7)


_EXACT = {}


def _exact_square_gradients(bank, seed):
    """gradients in {0, +-1}, a quarter of them non-zero: every partial sum of their squares is an integer below 2^24, exact in fp32 in
    ANY order -- the norm over two pieces is then the norm of one pass to the bit, and the comparison below can ask for equal bits"""
    n = bank.grad.numel()
    if (n, seed) not in _EXACT:
        gen = torch.Generator().manual_seed(seed)
        g = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).float() * (torch.rand(n, generator=gen) < 0.25)
        assert 0 < float(g.double().pow(2).sum()) < 2 ** 24
        _EXACT[(n, seed)] = g
    return _EXACT[(n, seed)]


@pytest.mark.parametrize("algo", ["adam", "adamax"])
def test_two_pieces_equal_one_whole_launch(hw, algo, dtype=torch.bfloat16):
    """launch(pieces=...) over a two-piece cover of [0, n_train) -- cut inside a parameter group, so that group is updated as two spans --
    and launch(grad16=...) with the same values as bf16: bit-identical masters, moments and bf16 copies to one whole fp32 launch"""
    _cfg, _sd, model = build("retrieval", RET, dtype, hw.dev)
    bank = model.rt.bank
    opt = OURS[algo](bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=0.5)
    a, b = max((pg["range"] for pg in opt.param_groups), key=lambda r: r[1] - r[0])
    cut = a + (b - a) // 3 // 4 * 4 + 4                                      # (spans start on whole f32x4 chunks, as GradSync's pieces do)
    assert a < cut < b
    start = _bank_state(bank)
    outs = []
    for mode in ("whole", "pieces", "grad16"):
        _restore(bank, start)
        opt.step_count = 0
        for step in range(2):
            opt.zero_grad()
            g = _exact_square_gradients(bank, 3 + step).to(hw.dev)
            bank.grad.copy_(g)
            if mode == "whole":
                opt.step()
            elif mode == "pieces":
                opt.step(pieces=[(0, cut), (cut, bank.n_train)], norm_reduce=lambda sq: None)
                bank.set_owner_only_dirty(False)                             # (the two pieces are the whole: nothing to gather)
            else:
                opt.step(grad16=g.bfloat16())
            assert opt.grad_norm() > 0.5                                     # the clip is active
        outs.append(_bank_state(bank))
    assert float((outs[0][0] - start[0]).abs().max()) > 1e-4
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert torch.equal(x, y)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["adam", "adamax"])
def test_captured_launch_equals_eager_steps(algo):
    """launch() captured once into a graph, prepare_step() eager before each of three replays: the masters of three eager steps, bit for bit"""
    dev = torch.device("cuda", 0)
    _cfg, _sd, model = build("retrieval", RET, torch.bfloat16, dev)
    bank = model.rt.bank
    opt = OURS[algo](bank, lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=0.5)
    grads = [_rnd(bank.grad.numel(), 40 + s).to(dev) for s in range(3)]
    start = _bank_state(bank)
    opt.zero_grad()
    for g in grads:                                                          # eager
        bank.grad.copy_(g)
        opt.step()
    eager = _bank_state(bank)
    _restore(bank, start)
    opt.step_count = 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.launch()
    for g in grads:
        bank.grad.copy_(g)
        opt.prepare_step()
        graph.replay()
    torch.cuda.synchronize()
    assert opt.step_count == 3 and float((eager[0] - start[0]).abs().max()) > 1e-4
    for x, y in zip(eager, _bank_state(bank)):
        assert torch.equal(x, y)


# ---- config and checkpoint (host emulator) ------------------------------------------------------------------------------------------

def _task_config(tmp_path, **over):
    model_json = dict(max_temporal_position_embeddings=100, backbone_channel_in_size=2048, max_grid_row_position_embeddings=100,
                      max_grid_col_position_embeddings=100, attention_probs_dropout_prob=0.1, hidden_act="gelu", hidden_dropout_prob=0.1,
                      hidden_size=128, initializer_range=0.02, intermediate_size=256, layer_norm_eps=1e-12, max_position_embeddings=32,
                      model_type="bert", num_attention_heads=2, num_hidden_layers=2, pad_token_id=0, type_vocab_size=2, vocab_size=200)
    (tmp_path / "model.json").write_text(json.dumps(model_json))
    task_json = dict(model_config=str(tmp_path / "model.json"), detectron2_model_cfg="R-50-grid.yaml", num_frm=2, train_n_clips=1,
                     learning_rate=1e-4, cnn_learning_rate=2e-5, weight_decay=1e-3, cnn_weight_decay=1e-4, grad_norm=5.0, loss_type="ce",
                     transformer_lr_mul=2.0, cnn_lr_mul=3.0, **over)
    (tmp_path / "task.json").write_text(json.dumps(task_json))
    return C.load_task_config(str(tmp_path / "task.json"), task="video_retrieval")


def test_setup_optimizer_builds_the_three_choices(tmp_path, emul):
    cfg = _task_config(tmp_path)
    model = C.setup_model(cfg, device=torch.device("cpu"), dtype=torch.float32)
    for name, eps in (("adam", 1e-8), ("adamax", 1e-8), ("adamw", 1e-6)):
        cfg.optim = name
        opt = C.setup_optimizer(model, cfg)
        assert type(opt) is OURS[name] and opt.algo == name
        assert len(opt.param_groups) == 8 and opt.eps == eps and opt.max_grad_norm == 5.0
        lrs = [g["lr"] for g in opt.param_groups]
        assert lrs[2] == pytest.approx(1e-4) and lrs[6] == pytest.approx(2e-5) and lrs[4] == pytest.approx(3.0 * 2e-5)
        assert sorted({g["weight_decay"] for g in opt.param_groups}) == [0.0, 1e-4, 1e-3]
    cfg.optim = "sgd"
    with pytest.raises(ValueError, match="invalid optimizer"):
        C.setup_optimizer(model, cfg)


def test_state_dict_round_trip_names_and_algo_check(emul):
    dev = torch.device("cpu")
    _cfg, _sd, model = build("retrieval", RET, torch.float32, dev)
    _cfg, _sd, model2 = build("retrieval", RET, torch.float32, dev)
    bank, bank2 = model.rt.bank, model2.rt.bank
    kw = dict(lr=1e-3, betas=(0.9, 0.98), weight_decay=1e-3, cnn_lr=1e-3, max_grad_norm=0.5)
    g1, g2 = _rnd(bank.grad.numel(), 50), _rnd(bank.grad.numel(), 51)
    start = None
    files = {}
    for algo in ("adam", "adamax", "adamw"):
        opt = OURS[algo](bank, **kw)
        start = start or _bank_state(bank)
        _restore(bank, start)
        bank.grad.copy_(g1)
        opt.step()
        sd = opt.state_dict()
        files[algo] = sd
        assert sd["algo"] == algo and sd["step"] == 1
        one = sd["state"]["transformer.bert.pooler.dense.weight"]
        second = "exp_inf" if algo == "adamax" else "exp_avg_sq"
        assert set(one) == {"step", "exp_avg", second} and one[second].shape == (128, 128) and float(one[second].abs().max()) > 0
        # into a fresh optimizer on a second bank holding the same weights: one more step, the same bits
        opt2 = OURS[algo](bank2, **kw)
        bank2.master.copy_(bank.master)
        opt2.load_state_dict(sd)
        assert opt2.step_count == 1
        for b, o in ((bank, opt), (bank2, opt2)):
            b.grad.copy_(g2)
            o.step()
        for (name, q), (_n2, q2) in zip(model.named_parameters(), model2.named_parameters()):
            assert torch.equal(q, q2), name
        a, b = opt.state_dict(), opt2.state_dict()
        assert a["step"] == b["step"] == 2
        for name, st in a["state"].items():
            assert torch.equal(st["exp_avg"], b["state"][name]["exp_avg"]) and torch.equal(st[second], b["state"][name][second]), name
        bank2.exp_avg.zero_()
        bank2.exp_avg_sq.zero_()
    with pytest.raises(ValueError, match="adamax"):
        optim.FusedAdam(bank2, **kw).load_state_dict(files["adamax"])
    with pytest.raises(ValueError, match="adam"):
        optim.FusedAdamW(bank2, **kw).load_state_dict(files["adam"])
    with pytest.raises(ValueError, match="adamw"):
        optim.FusedAdamax(bank2, **kw).load_state_dict(files["adamw"])
    old = {k: v for k, v in files["adamw"].items() if k != "algo"}           # a file written before the key existed is AdamW's
    w = optim.FusedAdamW(bank2, **kw)
    w.load_state_dict(old)
    assert w.step_count == 1
    assert float(bank2.exp_avg_sq.abs().max()) > 0
    with pytest.raises(ValueError, match="adamw"):
        optim.FusedAdam(bank2, **kw).load_state_dict(old)
