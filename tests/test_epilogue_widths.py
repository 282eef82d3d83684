"""The generic cb_gemm epilogue is ONE function for its three widths (csrc/gemm_epilogue.h epilogue_cols<T, W>): the same small problem,
M = 70, N = 64, K = 96 on the 64x64 tile (tile=2: the column tile is full, the second row tile ragged), goes through all three and must give
the same bits.  Which width runs is decided by gemm_prepare (csrc/gemm.hip) from the leading dimensions and base alignment of C, C2,
residual, mask and gelu_grad_pre alone:

    // vector epilogue: every touched row pointer must be 16-byte (fp32) / 8-byte (bf16) aligned at n%4==0
    bool cv = (d->ldc % 4 == 0) && ((reinterpret_cast<uintptr_t>(d->C) % (4 * cesz)) == 0);          [... the same for each operand]
    // row-contiguous epilogue: 8-wide chunks must be 16-byte aligned everywhere
    bool cv8 = cv && (d->N % 8 == 0) && (d->ldc % 8 == 0) && aligned16(d->C);                         [... the same for each operand]

and tile_epilogue: `if (p.c_vec8) W = 8; else if (p.split_k > 1 && p.c_vec) row-coalesced atomics; else if (p.c_vec && n0 + BN <= N) W = 4;
else W = 1`.  So with every buffer at one pitch `ld` (allocations are 64-byte aligned): ld = 72 -> W = 8, ld = 68 -> W = 4, ld = 67 -> W = 1.
The option rows below each miss the list of specialised bodies (FAST_EPI_COMBOS) on purpose, so that the bf16 ld = 72 call runs the
generic chain too.  The W = 8 result is also held to the bound of tests/test_kernels_gemm.py against an fp64 restatement of the chain.
Emulator build on CPU, the real library on `gpu`."""
import math

import pytest
import torch

import dropout_restatement as DR
from clipbert_amd import ops
from test_kernels_gemm import rnd, tol

M, N, K = 70, 64, 96
LDS = {8: 72, 4: 68, 1: 67}                 # width -> pitch of every M x N buffer
SENTINEL = -7.0
RES_ROWS = 40                               # rows of the compact residual behind res_rowmap
P_DROP, SEED, WORD = 0.3, 41, 1 << 33

# every branch of the chain at least once; keys: alpha, scale, shift, act, out2, dropout, residual, res_rowmap, c_rowmap, relu_after, mask,
# pre (gelu_grad_pre), accumulate, c_f32, relu_bwd, post_scale, post_scale2, split_k
CASES = {
    "alpha_scale": dict(alpha=0.5, scale=True),
    "shift_tanh": dict(shift=True, act=ops.ACT_TANH),
    "scale_shift_gelu": dict(scale=True, shift=True, act=ops.ACT_GELU),
    "shift_relu_out2": dict(shift=True, act=ops.ACT_RELU, out2=True),                       # C2 = the value before the activation
    "save_grad_residual": dict(shift=True, act=ops.ACT_GELU_SAVE_GRAD, out2=True, residual=True),
    "save_grad_without_out2": dict(scale=True, act=ops.ACT_GELU_SAVE_GRAD),                 # (a plain GELU)
    "dropout_residual": dict(shift=True, act=ops.ACT_TANH, dropout=True, residual=True),
    "res_rowmap_relu_after": dict(scale=True, residual=True, res_rowmap=True, relu_after=True),
    "c_rowmap": dict(shift=True, residual=True, c_rowmap=True),
    "mask": dict(shift=True, mask=True),
    "saved_grad": dict(scale=True, pre=True, act=ops.ACT_SAVED_GRAD),
    "gelu_grad_pre": dict(pre=True),
    "accumulate": dict(shift=True, accumulate=True),
    "accumulate_f32": dict(scale=True, accumulate=True, c_f32=True),
    "relu_bwd": dict(relu_bwd=True, mask=True, post_scale=True),
    "relu_bwd_all": dict(relu_bwd=True, mask=True, residual=True, out2=True, post_scale=True, post_scale2=True, accumulate=True),
    "split_k_atomics": dict(alpha=0.5, scale=True, accumulate=True, c_f32=True, split_k=2, zero_c=True),
}


def _inputs(dt, spec):
    """the operands of a case as compact CPU tensors (the same values whatever the pitch)"""
    t = dict(x=rnd(M, K, seed=1).to(dt), w=rnd(N, K, seed=2, scale=0.2).to(dt), scale=rnd(N, seed=3) * 0.5 + 1.0, shift=rnd(N, seed=4),
             residual=rnd(RES_ROWS if spec.get("res_rowmap") else M, N, seed=5).to(dt), mask=rnd(M, N, seed=6).to(dt), pre=rnd(M, N, seed=7).to(dt),
             post_scale=rnd(N, seed=8), post_scale2=rnd(N, seed=9))
    cdt = torch.float32 if spec.get("c_f32") else dt
    t["c_old"] = torch.zeros(M, N, dtype=cdt) if spec.get("zero_c") else rnd(M, N, seed=10).to(cdt)
    g = torch.Generator().manual_seed(11)
    t["c_rowmap"] = torch.randperm(M, generator=g).to(torch.int32)
    rm = torch.randint(0, RES_ROWS, (M,), generator=g).to(torch.int32)
    rm[torch.rand(M, generator=g) < 0.25] = -1
    t["res_rowmap"] = rm
    return t


def _pitched(t, ld, dev):
    buf = torch.full((t.shape[0], ld), SENTINEL, dtype=t.dtype)
    buf[:, :N] = t
    return buf.to(dev)


def _run(hw, dt, spec, t, ld):
    """one cb_gemm call with every M x N buffer at pitch ld -> (C, C2 or None) valid regions on the CPU; checks the padding columns"""
    on = lambda k: spec.get(k, False)                                                             # noqa: E731
    out = _pitched(t["c_old"], ld, hw.dev)
    out2 = _pitched(torch.zeros(M, N, dtype=dt), ld, hw.dev) if on("out2") else None
    kw = dict(out=out, tile=2, alpha=spec.get("alpha", 1.0), act=spec.get("act", ops.ACT_NONE), out2=out2, accumulate=on("accumulate"),
              relu_after=on("relu_after"), relu_bwd=on("relu_bwd"), split_k=spec.get("split_k", 1))
    for k in ("scale", "shift", "post_scale", "post_scale2"):
        kw[k] = hw(t[k]) if on(k) else None
    for k, name in (("residual", "residual"), ("mask", "mask"), ("pre", "gelu_grad_pre")):
        kw[name] = _pitched(t[k], ld, hw.dev) if on(k) else None
    for k in ("c_rowmap", "res_rowmap"):
        kw[k] = hw(t[k]) if on(k) else None
    if on("dropout"):
        kw.update(dropout_p=P_DROP, dropout_seed=SEED, seed_ptr=torch.tensor([WORD], dtype=torch.int64, device=hw.dev))
    ops.gemm(hw(t["x"]), hw(t["w"]), M, N, K, **kw)
    for buf in (out, out2):
        assert buf is None or bool((buf[:, N:].cpu() == SENTINEL).all()), "padding columns were written"
    return out[:, :N].cpu(), None if out2 is None else out2[:, :N].cpu()


def _gelu64(v):
    cdf = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def _restate(spec, t):
    """the option chain in fp64, in the order include/clipbert_hip.h gives it -> (C, C2 or None)"""
    on = lambda k: spec.get(k, False)                                                             # noqa: E731
    d = {k: v.double() for k, v in t.items()}
    orow = t["c_rowmap"].long() if on("c_rowmap") else torch.arange(M)                             # row m lives at C / C2 / mask / pre row orow[m]
    res = None
    if on("residual") and on("res_rowmap"):
        rm = t["res_rowmap"].long()
        res = torch.where((rm >= 0)[:, None], d["residual"][rm.clamp(min=0)], torch.zeros(M, N, dtype=torch.float64))
    elif on("residual"):
        res = d["residual"][orow]
    v = spec.get("alpha", 1.0) * (d["x"] @ d["w"].t())
    c2 = None
    if on("relu_bwd"):
        if on("accumulate"):
            v = v + d["c_old"][orow]
        if res is not None:
            v = v + res
        v = torch.where(d["mask"][orow] > 0, v, torch.zeros_like(v))
        c2 = v * d["post_scale2"] if on("post_scale2") else v
        v = v * d["post_scale"] if on("post_scale") else v
    else:
        if on("scale"):
            v = v * d["scale"]
        if on("shift"):
            v = v + d["shift"]
        act = spec.get("act", ops.ACT_NONE)
        if act == ops.ACT_GELU_SAVE_GRAD and on("out2"):
            v, c2 = _gelu64(v)
        else:
            c2 = v
            v = {ops.ACT_NONE: v, ops.ACT_SAVED_GRAD: v, ops.ACT_RELU: torch.relu(v), ops.ACT_TANH: torch.tanh(v), ops.ACT_GELU: _gelu64(v)[0],
                 ops.ACT_GELU_SAVE_GRAD: _gelu64(v)[0]}[act]
        if on("dropout"):
            v = v * DR.mult_mask(DR.effective_seed(SEED, WORD), M, N, P_DROP)
        if res is not None:
            v = v + res
        if on("relu_after"):
            v = torch.relu(v)
        if on("mask"):
            v = torch.where(d["mask"][orow] > 0, v, torch.zeros_like(v))
        if on("pre"):
            v = v * (d["pre"][orow] if act == ops.ACT_SAVED_GRAD else _gelu64(d["pre"][orow])[1])
        if on("accumulate"):
            v = v + d["c_old"][orow]
    c = d["c_old"].clone()
    c[orow] = v
    if not on("out2"):
        return c, None
    full2 = torch.zeros(M, N, dtype=torch.float64)
    full2[orow] = c2
    return c, full2


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("case", list(CASES))
def test_three_widths_give_the_same_bits(hw, monkeypatch, dt, case):
    spec = CASES[case]
    if spec.get("split_k", 1) > 1:
        monkeypatch.setattr(ops, "_SPLITK_OFF", True)            # no K-split scratch: the parts combine through fp32 atomics (two addends onto zero: exact)
    t = _inputs(dt, spec)
    got = {w: _run(hw, dt, spec, t, ld) for w, ld in LDS.items()}
    ref = _restate(spec, t)
    for i, name in enumerate(("C", "C2")):
        if ref[i] is None:
            assert got[8][i] is None
            continue
        for w in (4, 1):
            assert torch.equal(got[w][i], got[8][i]), f"{name}: width {w} differs from width 8"
        torch.testing.assert_close(got[8][i].double(), ref[i], **tol(dt))


@pytest.mark.parametrize("ld", list(LDS.values()))
def test_mask_with_gelu_grad_pre_is_refused(hw, ld):
    dt = torch.bfloat16
    t = _inputs(dt, {})
    out = _pitched(t["c_old"], ld, hw.dev)
    with pytest.raises(RuntimeError, match="exclude each other"):
        ops.gemm(hw(t["x"]), hw(t["w"]), M, N, K, out=out, tile=2, mask=_pitched(t["mask"], ld, hw.dev), gelu_grad_pre=_pitched(t["pre"], ld, hw.dev))
    assert bool((out.cpu()[:, :N] == t["c_old"]).all())
