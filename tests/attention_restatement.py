"""float64 restatement of the self-attention kernels (clipbert_amd/csrc/attention.hip, attention_mfma.hip) with the bf16 roundings of each
route put where the kernel puts them, the worst-case error bounds that follow from those roundings, and the inputs of the exact routing
probes.  Test infrastructure only: plain torch on the CPU, used by test_attention_budget.py.  No tests in here.

R(x) is round-to-nearest-even to bf16.  m is the dropout multiplier matrix (dropout_restatement.attention_mult; ones without dropout).

    s = q k^T / 8 + (1 - mask) * -10000         p = softmax(s)        lse = logsumexp(s)
    backward, from the ctx and lse it is GIVEN:   P = exp(s - lse)   D_i = sum_d dO_id ctx_id   dP = dO v^T   dS = P (dP m - D) / 8

                 MFMA routes (every pack_pair() call site)       generic route (fp32 throughout, outputs rounded)
    ctx          R( R(p m) v )                                   R( (p m) v )
    dq           R( R(dS) k )                                    R( dS k )
    dk           R( R(dS)^T q )                                  R( dS^T q )
    dv           R( R(P m)^T dO )                                R( (P m)^T dO )

route "exact" is the same arithmetic without any R.

Bounds (bounds() below), u = 2^-8 the bf16 unit round-off, DELTA = 2^-16 the allowance for fp32 arithmetic and the fast-math exp / log /
reciprocal; on the generic route the u inside the sums and inside E goes (nothing is rounded there):
    ctx  u |o|  + (u + DELTA) sum_j p_ij m_ij |v_jd|
    E_ij = u |dS_ij| + DELTA P_ij (|dP_ij| m_ij + |D_i|) / 8
    dq   u |dq| + sum_j E_ij |k_jd|          dk   u |dk| + sum_i E_ij |q_id|
    dv   u |dv| + (u + DELTA) sum_i P_ij m_ij |dO_id|

Measured (test_attention_budget.py; B = 2, H = 3 and the (1, 12), (3, 1) shapes, Q as drawn and Q x 3, with and without dropout), the largest
figure over the cases of a route.  share = fraction of the elements of one output tensor that differ from the route's restatement (cap 1e-2);
ratio = |got - exact| / bound (cap 1.02); lse = |lse - logsumexp| / max(1, |lse|) (cap 4e-6); other = smallest share against the OTHER
route's restatement at L >= 41 (floor 0.1).

                share, emulator        share, MI355X          ratio, emulator    ratio, MI355X
    route       ctx      dq/dk/dv      ctx      dq/dk/dv      ctx   dq/dk/dv     ctx   dq/dk/dv
    mfma<1>     0        1.6e-4        0        1.6e-4        0.87  0.85         0.87  0.85
    mfma<2>     0        7.3e-4        0        7.3e-4        0.80  0.82         0.80  0.82
    mfma<3>     3.2e-5   9.8e-4        5.4e-5   9.8e-4        0.86  0.82         0.86  0.82
    mfma<4>     1.1e-4   1.3e-3        1.2e-4   1.8e-3        0.86  0.84         0.86  0.84
    big<6>      3.0e-4   1.3e-3        6.5e-4   1.3e-3        0.87  0.82         0.87  0.82
    big<8>      1.0e-3   3.3e-4        1.0e-3   1.2e-3        0.82  0.80         0.82  0.80
    big<10>     7.2e-4   8.8e-4        8.5e-4   6.5e-4        0.94  0.84         0.94  0.84
    big<12>     3.9e-4   9.9e-4        8.1e-4   1.0e-3        0.82  0.78         0.82  0.78
    generic     3.0e-4   4.2e-4        3.0e-4   4.5e-4        0.99  0.99         0.99  0.99
    lse: 1.7e-7 on the emulator, 2.2e-7 on the MI355X.  other: 0.19 (dv of mfma<3> at L = 41, Q x 3, against the generic restatement), 0.28
    (the generic kernels against the MFMA restatement, same tensor and case), 0.29 .. 0.36 on every other route; the same on both backends.
The device's fast-math exp, log and reciprocal move the share by less than 1e-3 anywhere, so the cap of 1e-2 holds for both backends.  The
generic route sits at 0.99 of its bound because the bound there is little more than the half ulp of the output rounding (u |x| is attained
just above a power of two), not because fp32 noise uses the allowance up.
Mutants, on the emulator: pack_pair() truncating instead of rounding changes 0.80 .. 0.83 of the elements on every MFMA route and fails (a)
and (c) (ratio 1.6 .. 1.8) in every case but L = 1, whose results are exactly representable; sending the <10> sizes to the <8> instance
fails both probes and the budget at L = 129, 145, 160; sending them to <12> (a legal over-padding) passes; reading the neighbour's key-mask
element in the forward of the register-resident kernels fails both probes and the budget at every L from 9 to 64.

Exact probes: keys are +-1 codes of length 64, q_i = 64 code(target of i), V and dO integers in [-4, 4].  The target's score is 64 * 64 / 8 =
512 (one-hot) or 64 * 48 / 8 = 384 (a decoy: its masked original with the first 8 signs flipped), every other unmasked key is at least
MARGIN = 110 below, so its probability underflows to 0 in fp32 (exp(-104) is already below half the smallest denormal) and nothing in either
pass rounds: ctx_i = v_target, lse = the target's score, dq = dk = 0, dv_j = the sum of dO_i over the queries aimed at j."""
import torch

U = 2.0 ** -8                                               # bf16 unit round-off
DELTA = 2.0 ** -16                                          # fp32 + fast-math allowance
MASK_NEG = -10000.0
MARGIN = 110.0
DH = 64


def R(x: torch.Tensor) -> torch.Tensor:
    return x.float().bfloat16().double()


def _id(x):
    return x


def split(qkv: torch.Tensor, B: int, L: int, H: int):
    """(B * L, 3 * H * 64) -> q, k, v float64 (B, H, L, 64)"""
    x = qkv.detach().cpu().double().view(B, L, 3, H, DH)
    return [x[:, :, i].permute(0, 2, 1, 3) for i in range(3)]


def heads(x: torch.Tensor, B: int, L: int, H: int) -> torch.Tensor:
    """(B * L, H * 64) -> float64 (B, H, L, 64)"""
    return x.detach().cpu().double().view(B, L, H, DH).permute(0, 2, 1, 3)


def rows(x: torch.Tensor) -> torch.Tensor:
    """(B, H, L, 64) -> (B * L, H * 64)"""
    B, H, L, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * L, H * DH)


def scores(q, k, mask) -> torch.Tensor:
    return q @ k.transpose(-1, -2) / 8.0 + ((1.0 - mask.detach().cpu().double()) * MASK_NEG)[:, None, None, :]


def _mult(m, s):
    return torch.ones_like(s) if m is None else m.double()


def forward(qkv, mask, B, L, H, m=None, route="exact"):
    """-> ctx float64 (B * L, H * 64), lse float64 (B, H, L)"""
    r_in = R if route == "mfma" else _id
    r_out = _id if route == "exact" else R
    q, k, v = split(qkv, B, L, H)
    s = scores(q, k, mask)
    pm = torch.softmax(s, -1) * _mult(m, s)
    return r_out(rows(r_in(pm) @ v)), torch.logsumexp(s, -1)


def backward(qkv, mask, ctx, lse, dctx, B, L, H, m=None, route="exact"):
    """-> dqkv float64 (B * L, 3 * H * 64), from the ctx (B * L, H * 64) and lse (B * H * L) of a forward pass"""
    r_in = R if route == "mfma" else _id
    r_out = _id if route == "exact" else R
    q, k, v = split(qkv, B, L, H)
    o, g = heads(ctx, B, L, H), heads(dctx, B, L, H)
    s = scores(q, k, mask)
    mm = _mult(m, s)
    P = torch.exp(s - lse.detach().cpu().double().view(B, H, L, 1))
    D = (g * o).sum(-1, keepdim=True)
    dS = P * (g @ v.transpose(-1, -2) * mm - D) / 8.0
    dq = r_in(dS) @ k
    dk = r_in(dS).transpose(-1, -2) @ q
    dv = r_in(P * mm).transpose(-1, -2) @ g
    return r_out(torch.cat([rows(dq), rows(dk), rows(dv)], 1))


def bounds(qkv, mask, ctx, lse, dctx, B, L, H, m=None, route="mfma"):
    """-> (ctx bound (B * L, H * 64), dqkv bound (B * L, 3 * H * 64)) on |kernel - exact|; the forward's from the exact p, the backward's from
    the given ctx and lse (module docstring)"""
    u_in = U if route == "mfma" else 0.0
    q, k, v = split(qkv, B, L, H)
    o, g = heads(ctx, B, L, H), heads(dctx, B, L, H)
    s = scores(q, k, mask)
    mm = _mult(m, s)
    pm = torch.softmax(s, -1) * mm
    b_ctx = U * (pm @ v).abs() + (u_in + DELTA) * (pm @ v.abs())
    P = torch.exp(s - lse.detach().cpu().double().view(B, H, L, 1))
    D = (g * o).sum(-1, keepdim=True)
    dP = g @ v.transpose(-1, -2)
    dS = P * (dP * mm - D) / 8.0
    E = u_in * dS.abs() + DELTA * P * (dP.abs() * mm + D.abs()) / 8.0
    b_dq = U * (dS @ k).abs() + E @ k.abs()
    b_dk = U * (dS.transpose(-1, -2) @ q).abs() + E.transpose(-1, -2) @ q.abs()
    b_dv = U * ((P * mm).transpose(-1, -2) @ g).abs() + (u_in + DELTA) * ((P * mm).transpose(-1, -2) @ g.abs())
    return rows(b_ctx), torch.cat([rows(b_dq), rows(b_dk), rows(b_dv)], 1)


def key_mask(B: int, L: int) -> torch.Tensor:
    """fp32 (B, L): batch 0 has its last min(3, L - 1) keys masked; the last batch entry key 0 and, for L > 32, the whole tile 16..31"""
    mask = torch.ones(B, L)
    n = min(3, L - 1)
    if n:
        mask[0, L - n:] = 0
    mask[B - 1, 0] = 0
    if L > 32:
        mask[B - 1, 16:32] = 0
    return mask


def _probe_head(L, keep, decoy, gen):
    """one (batch, head): codes (L, 64) of +-1, target (L,) the key every query is aimed at, top the target's raw score"""
    idx = torch.arange(L)
    unm, msk = idx[keep], idx[~keep]
    codes = (torch.randint(0, 2, (L, DH), generator=gen) * 2 - 1).double()
    if decoy and 0 < len(msk) <= len(unm):
        d = unm[torch.randperm(len(unm), generator=gen)[:len(msk)]]
        codes[d] = codes[msk]
        codes[d, :8] *= -1
        aim = msk[idx % len(msk)]                           # the raw best key of query i is a masked one ...
        target = d[idx % len(msk)]                          # ... and its decoy must win
        return codes, aim, target
    cand = unm if len(unm) else idx                         # every key masked: the mask shifts all scores alike
    target = torch.empty(L, dtype=torch.long)
    inside = torch.zeros(L, dtype=torch.bool)
    inside[cand] = True
    target[cand] = cand[torch.randperm(len(cand), generator=gen)]
    rest = idx[~inside]
    target[rest] = cand[torch.arange(len(rest)) % len(cand)]
    return codes, target, target


def probe(B: int, L: int, H: int, mask: torch.Tensor, decoy: bool, seed: int = 0):
    """-> dict of float64 tensors: qkv (B * L, 3 * H * 64), dctx (B * L, H * 64), target int64 (B, H, L), and the exact results ctx, lse
    (B, H, L), dqkv.  A head whose draw misses MARGIN is drawn again (a random code pair correlates that much once in ~1e5)."""
    gen = torch.Generator().manual_seed(1000 * L + seed)
    q, k = torch.empty(B, H, L, DH, dtype=torch.float64), torch.empty(B, H, L, DH, dtype=torch.float64)
    target = torch.empty(B, H, L, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            for _ in range(64):
                codes, aim, tgt = _probe_head(L, mask[b] > 0, decoy, gen)
                k[b, h], q[b, h], target[b, h] = codes, 64.0 * codes[aim], tgt
                if float(top2_gap(scores(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], mask[b:b + 1])).min()) >= MARGIN:
                    break
    v = torch.randint(-4, 5, (B, H, L, DH), generator=gen).double()
    g = torch.randint(-4, 5, (B, H, L, DH), generator=gen).double()
    s = scores(q, k, mask)
    ctx = torch.gather(v, 2, target[..., None].expand(-1, -1, -1, DH))
    dv = torch.zeros_like(v).scatter_add_(2, target[..., None].expand(-1, -1, -1, DH), g)
    return dict(qkv=torch.cat([rows(q), rows(k), rows(v)], 1), dctx=rows(g), target=target, scores=s, ctx=rows(ctx),
                lse=torch.gather(s, 3, target[..., None])[..., 0], dqkv=torch.cat([torch.zeros(B * L, 2 * H * DH, dtype=torch.float64), rows(dv)], 1))


def top2_gap(s: torch.Tensor) -> torch.Tensor:
    """best minus second-best score of every query (inf for a single key)"""
    if s.shape[-1] == 1:
        return torch.full(s.shape[:-1], float("inf"), dtype=torch.float64)
    top = s.topk(2, dim=-1)[0]
    return top[..., 0] - top[..., 1]
