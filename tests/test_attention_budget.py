"""cb_attention_fwd / _bwd held to the rounding points of the route that serves the call (attention_restatement.py): on random bf16 data
the share of elements that differ from the route's float64 restatement, a derived worst-case bound on every element and the lse; on
exact probes (one-hot and masked-decoy scores, integer values) every element of both passes, bf16 and fp32.  The cases are the smallest
shapes on each side of every route boundary of attention_mfma.hip, and the generic kernels behind operands that are not 16-byte aligned.
Each case runs on the host emulator build and, marked `gpu`, on the device."""
import functools

import pytest
import torch

import attention_restatement as AR
import dropout_restatement as DR
from clipbert_amd import ops

B0, H0 = 2, 3                                               # H odd, so a b / h mix-up shows
LS = [1, 9, 16, 17, 32, 41, 48, 49, 64, 65, 69, 80, 96, 112, 128, 129, 145, 160, 169, 192, 193, 200, 257]
LS_DROP = [20, 41, 64, 69, 145, 169, 200]
PLAIN, ALL_OFF, DQ_OFF = "plain", "qkv_ctx_off8", "dqkv_off8"
CASES = [(L, B0, H0, PLAIN) for L in LS] + [(41, 1, 12, PLAIN), (41, 3, 1, PLAIN)] + [(L, B0, H0, a) for a in (ALL_OFF, DQ_OFF) for L in (41, 69)]
SHARE_CAP = 1e-2                                            # (a)
OTHER_FLOOR = 0.1                                           # (b)
BOUND_SLACK = 1.02                                          # (c)
LSE_TOL = 4e-6                                              # (d)
DROP_P, DROP_SEED, DROP_WORD = 0.1, 5, 11


def route_name(L, aligned=True):
    if L > 192 or not aligned:
        return "generic"
    nt = (L + 15) // 16
    return f"mfma<{nt}>" if nt <= 4 else f"big<{(nt + 1) // 2 * 2}>"


def off8(shape, dtype, dev):
    """a tensor of this shape 8 bytes into a larger buffer: not 16-byte aligned, so the MFMA kernels decline it, still aligned for the
    4-element loads of the generic ones"""
    n = 1
    for s in shape:
        n *= s
    assert dtype == torch.bfloat16
    t = torch.zeros(n + 8, dtype=dtype, device=dev)[4:4 + n].view(shape)
    assert t.data_ptr() % 16 == 8
    return t


@functools.lru_cache(maxsize=None)
def random_case(L, B, H, scale):
    """bf16 inputs (CPU, shared by both backends and never written to): qkv with Q x scale, dctx, key mask"""
    qkv = torch.randn(B * L, 3, H * 64, generator=torch.Generator().manual_seed(1))
    qkv[:, 0] *= scale
    dctx = torch.randn(B * L, H * 64, generator=torch.Generator().manual_seed(2))
    return qkv.view(B * L, 3 * H * 64).bfloat16(), dctx.bfloat16(), AR.key_mask(B, L)


def share(got, want):
    return float((got != want).double().mean())


def thirds(x):
    return dict(zip(("dq", "dk", "dv"), x.view(x.shape[0], 3, -1).unbind(1)))


def run_budget(hw, L, B, H, scale, place, p=0.0):
    qkv16, dctx16, mask = random_case(L, B, H, scale)
    dev = hw.dev
    sp = torch.tensor([DROP_WORD], dtype=torch.int64, device=dev) if p else None
    kw = dict(dropout_p=p, dropout_seed=DROP_SEED, seed_ptr=sp) if p else {}
    m = DR.attention_mult(DR.effective_seed(DROP_SEED, DROP_WORD), B, H, L, p) if p else None
    qkv, ctx_out = hw(qkv16), None
    if place == ALL_OFF:
        qkv = off8(qkv16.shape, torch.bfloat16, dev).copy_(qkv16)
        ctx_out = off8((B * L, H * 64), torch.bfloat16, dev)
    dq_out = off8(qkv16.shape, torch.bfloat16, dev) if place == DQ_OFF else None
    fwd_route = route_name(L, place != ALL_OFF)
    bwd_route = route_name(L, place == PLAIN)
    ctx, lse = ops.attention_fwd(qkv, hw(mask), B, L, H, save_lse=True, out=ctx_out, **kw)
    dqkv = ops.attention_bwd(qkv, hw(mask), ctx, hw(dctx16), lse, B, L, H, out=dq_out, **kw)
    assert (ctx.data_ptr() % 16 == 0) == (place != ALL_OFF) and (dqkv.data_ptr() % 16 == 0) == (place != DQ_OFF)
    ctx, lse, dqkv = ctx.cpu(), lse.cpu(), dqkv.cpu()
    kind = {r: ("generic" if r == "generic" else "mfma") for r in (fwd_route, bwd_route)}
    other = {"mfma": "generic", "generic": "mfma"}

    got = dict(ctx=ctx.double(), **thirds(dqkv.double()))
    want, wrong, exact, bound = {}, {}, {}, {}
    for dst, r in ((want, kind[fwd_route]), (wrong, other[kind[fwd_route]]), (exact, "exact")):
        dst["ctx"], lse64 = AR.forward(qkv16, mask, B, L, H, m, r)
    for dst, r in ((want, kind[bwd_route]), (wrong, other[kind[bwd_route]]), (exact, "exact")):
        dst.update(thirds(AR.backward(qkv16, mask, ctx, lse, dctx16, B, L, H, m, r)))
    bound["ctx"], _ = AR.bounds(qkv16, mask, ctx, lse, dctx16, B, L, H, m, kind[fwd_route])
    bound.update(thirds(AR.bounds(qkv16, mask, ctx, lse, dctx16, B, L, H, m, kind[bwd_route])[1]))

    lse_err = float(((lse.double().view(B, H, L) - lse64).abs() / lse64.abs().clamp(min=1.0)).max())
    shares = {n: share(got[n], want[n]) for n in got}
    others = {n: share(got[n], wrong[n]) for n in got}
    ratios = {n: float(((got[n] - exact[n]).abs() / bound[n].clamp(min=1e-300)).max()) for n in got}
    fmt = lambda d: " ".join(f"{n}={v:.3g}" for n, v in d.items())      # noqa: E731
    print(f"\nBUDGET hw={hw.name} fwd={fwd_route} bwd={bwd_route} L={L} B={B} H={H} scale={scale} p={p} place={place} lse={lse_err:.3g} "
          f"| share {fmt(shares)} | other {fmt(others)} | ratio {fmt(ratios)}")

    assert lse_err <= LSE_TOL, lse_err                                                  # (d)
    if L == 1:                                              # the exact dq, dk are 0 there and fp32 noise decides: exempt from (a)
        q, k, v = [AR.rows(t) for t in AR.split(qkv16, B, L, H)]
        assert torch.equal(got["ctx"], v) and torch.equal(got["dv"], dctx16.double())
        cap = 2.0 ** -20 * float(dctx16.abs().max()) * float(v.abs().max()) * float(k.abs().max()) * 64
        assert float(got["dq"].abs().max()) <= cap and float(got["dk"].abs().max()) <= cap
        shares.pop("dq"), shares.pop("dk")
    for n, v in shares.items():                                                         # (a)
        assert v <= SHARE_CAP, (n, v, fwd_route, bwd_route)
    if L >= 41:                                                                         # (b): which kernel ran
        for n, v in others.items():
            assert v > OTHER_FLOOR, (n, v, fwd_route, bwd_route)
    for n in got:                                                                       # (c); a zero bound demands an exact zero
        assert bool(((got[n] - exact[n]).abs() <= BOUND_SLACK * bound[n]).all()), (n, ratios[n], fwd_route, bwd_route)


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("L,B,H,place", CASES, ids=[f"L{c[0]}-B{c[1]}H{c[2]}-{c[3]}" for c in CASES])
def test_attention_rounding_budget(hw, L, B, H, place, scale):
    run_budget(hw, L, B, H, scale, place)


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("L", LS_DROP)
def test_attention_rounding_budget_dropout(hw, L, scale):
    run_budget(hw, L, B0, H0, scale, PLAIN, p=DROP_P)


@functools.lru_cache(maxsize=None)
def probe_case(L, decoy):
    return AR.probe(B0, L, H0, AR.key_mask(B0, L), decoy)


def run_probe(hw, dt, L, decoy):
    B, H = B0, H0
    mask = AR.key_mask(B, L)
    pr = probe_case(L, decoy)
    # what makes the probe valid: the target wins by MARGIN, so every other probability is 0 in fp32; and no sum leaves bf16's integers
    assert torch.equal(pr["scores"].argmax(-1), pr["target"])
    assert float(AR.top2_gap(pr["scores"]).min()) >= AR.MARGIN
    assert float(pr["dqkv"].abs().max()) <= 256
    if decoy and L > 1:                                     # every batch entry of this mask has masked keys and room for their decoys
        assert bool((pr["lse"] == 384).all()) and bool((mask.view(B, 1, L).expand(B, H, L).gather(2, pr["target"]) == 1).all())
    elif L > 1:
        assert bool((pr["lse"] == 512).all())
    qkv, dctx = hw(pr["qkv"].to(dt)), hw(pr["dctx"].to(dt))
    assert torch.equal(qkv.double().cpu(), pr["qkv"])
    ctx, lse = ops.attention_fwd(qkv, hw(mask), B, L, H, save_lse=True)
    dqkv = ops.attention_bwd(qkv, hw(mask), ctx, dctx, lse, B, L, H)
    assert torch.equal(ctx.double().cpu(), pr["ctx"])
    assert torch.equal(lse.double().cpu().view(B, H, L), pr["lse"])
    got = thirds(dqkv.double().cpu())
    for n, want in thirds(pr["dqkv"]).items():
        assert torch.equal(got[n], want), (n, float((got[n] - want).abs().max()))


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("L", LS)
def test_attention_one_hot_probe(hw, dt, L):
    """q_i = 64 code(pi(i)), pi a permutation of the unmasked keys (masked positions aim at them cyclically): ctx_i = v_pi(i), lse = 512,
    dq = dk = 0, dv_j = the sum of dO_i over pi(i) = j, all with torch.equal.  A swapped key tile, k-slot or b / h index names its element."""
    run_probe(hw, dt, L, decoy=False)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("L", LS)
def test_attention_masked_decoy_probe(hw, dt, L):
    """every query is 64 code(a) of a MASKED key a, whose copy with 8 signs flipped sits at an unmasked key d(a): the decoy must win, ctx_i =
    v_d(a) and lse = 384 exactly; a kernel that reads the wrong mask element returns v_a.  (L = 1 has no room for a decoy: one-hot there.)"""
    run_probe(hw, dt, L, decoy=True)
