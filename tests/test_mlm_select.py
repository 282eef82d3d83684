"""cb_mlm_select / cb_mlm_loss_fwd / cb_mlm_loss_bwd through clipbert_amd.ops: the device-side compaction of the labelled text rows against
a NumPy restatement, and the loss / arg-max / gradient of the compact logits against torch in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clipbert_amd import ops

IGN = -100


def select_restatement(labels, lt, l, d, v, cap):
    """cb_mlm_select as include/clipbert_hip.h words it"""
    labels = np.asarray(labels, dtype=np.int64)
    rows = labels.size
    lab = [r for r in range(rows) if labels[r] != IGN and 0 <= labels[r] < v]
    kept = lab[:cap]
    slot_row = np.full(cap, -1, np.int32)
    slot_label = np.full(cap, IGN, np.int64)
    off = np.zeros(cap, np.int32)
    ih0 = np.full(cap, -1, np.int16)
    iw0 = np.zeros(cap, np.int16)
    rowmap = np.full(cap, (rows // lt) * l, np.int32)
    for j, r in enumerate(kept):
        b, t = divmod(r, lt)
        slot_row[j], slot_label[j] = r, labels[r]
        off[j], ih0[j], iw0[j] = (b * l + t) * d, 0, t
        rowmap[j] = b * l + t
    return dict(slot_row=slot_row, slot_label=slot_label, off=off, ih0=ih0, iw0=iw0, rowmap=rowmap, count=len(lab), dropped=max(0, len(lab) - cap))


def check_select(hw, labels, lt, l, d, v, cap, counts=None, dropped_before=0):
    sel = ops.mlm_select(hw(torch.as_tensor(labels, dtype=torch.int64)), lt, l, d, v, cap, counts=counts)
    want = select_restatement(labels, lt, l, d, v, cap)
    tab = sel.tab.cpu().numpy().view(np.dtype([("off", np.int32), ("ih0", np.int16), ("iw0", np.int16)]))
    np.testing.assert_array_equal(sel.slot_row.cpu().numpy(), want["slot_row"])
    np.testing.assert_array_equal(sel.slot_label.cpu().numpy(), want["slot_label"])
    np.testing.assert_array_equal(tab["off"], want["off"])
    np.testing.assert_array_equal(tab["ih0"], want["ih0"])
    np.testing.assert_array_equal(tab["iw0"], want["iw0"])
    np.testing.assert_array_equal(sel.rowmap.cpu().numpy(), want["rowmap"])
    kept = min(want["count"], cap)
    rows = len(labels)
    assert (np.diff(want["slot_row"][:kept]) > 0).all()                                   # ascending row order
    assert (sel.rowmap.cpu().numpy()[kept:] == (rows // lt) * l).all()                    # padding -> the dump row, never a real one
    assert (sel.rowmap.cpu().numpy()[:kept] < (rows // lt) * l).all()
    assert sel.counts.cpu().tolist() == [want["count"], dropped_before + want["dropped"]]
    assert sel.loss_rows.shape == (rows,) and (sel.loss_rows.cpu() == 0).all()
    assert sel.pred_rows.shape == (rows,) and (sel.pred_rows.cpu() == IGN).all()
    return sel, want


def _patterns(rows, v):
    rng = np.random.default_rng(5)
    none = np.full(rows, IGN, np.int64)
    every = rng.integers(0, v, rows).astype(np.int64)
    ends = none.copy()
    ends[0], ends[-1] = 3, v - 1
    some = np.where(rng.random(rows) < 0.3, rng.integers(0, v, rows), IGN).astype(np.int64)
    bad = some.copy()
    bad[np.flatnonzero(some != IGN)[1]] = v                                               # out of range: treated as ignored
    bad[np.flatnonzero(some == IGN)[0]] = -7
    return dict(none=none, all=every, ends=ends, some=some, bad=bad)


@pytest.mark.parametrize("pattern", ["none", "all", "ends", "some", "bad"])
def test_select_matches_restatement(hw, pattern):
    b, lt, l, d, v = 3, 7, 11, 16, 200
    labels = _patterns(b * lt, v)[pattern]
    count = select_restatement(labels, lt, l, d, v, 64)["count"]
    assert count == {"none": 0, "all": 21, "ends": 2}.get(pattern, count)
    if pattern == "bad":
        assert count == int((_patterns(b * lt, v)["some"] != IGN).sum()) - 1
    for cap in sorted({max(count, 1), count + 1, 64}):
        check_select(hw, labels, lt, l, d, v, cap)


def test_select_overflow_keeps_the_first_rows_and_counts_the_rest(hw):
    b, lt, l, d, v = 3, 7, 11, 16, 200
    labels = np.full(b * lt, IGN, np.int64)
    labels[[0, 4, 9, 13, 20]] = [5, 6, 7, 8, 9]
    sel, want = check_select(hw, labels, lt, l, d, v, 2)
    assert want["slot_row"].tolist() == [0, 4] and sel.counts.cpu().tolist() == [5, 3]
    check_select(hw, labels, lt, l, d, v, 2, counts=sel.counts, dropped_before=3)         # counts[1] accumulates: [5, 6]
    check_select(hw, labels, lt, l, d, v, 5, counts=sel.counts, dropped_before=6)         # count == cap exactly: nothing more dropped


@pytest.mark.parametrize("rows", [64, 65, 1000])
def test_select_crosses_the_block_size(hw, rows):
    rng = np.random.default_rng(rows)
    lt, v = rows // 5 if rows % 5 == 0 else rows, 30522
    labels = np.where(rng.random(rows) < 0.3, rng.integers(0, v, rows), IGN).astype(np.int64)
    labels[-1] = 17                                                                       # the last row of the last chunk
    count = int((labels != IGN).sum())
    for cap in (count, count + 1, 64):
        check_select(hw, labels, lt, lt + 9, 768, v, cap)


# ---- loss forward / backward ------------------------------------------------------------------------------------------------------

def _loss_case(hw, slots, v, ld, seed=0, misalign=0):
    """``slots`` labelled rows + one padding slot; logits (slots + 1, v) with row stride ld, pad columns +1e30; one row with a two-way tie"""
    g = torch.Generator().manual_seed(seed)
    cap, rows = slots + 1, slots + 3
    labels = torch.full((rows,), IGN, dtype=torch.int64)
    where = torch.randperm(rows, generator=g)[:slots].sort().values
    labels[where] = torch.randint(0, v, (slots,), generator=g)
    store = torch.full((cap * ld + misalign,), 1e30)
    view = store[misalign:].view(cap, ld)
    view[:, :v] = torch.randn(cap, v, generator=g) * 3
    lo, hi = (1, v - 2) if v > 3 else (0, v - 1)
    tie_row = slots - 1
    view[tie_row, lo] = view[tie_row, hi] = view[tie_row, :v].max() + 1.0
    logits = hw(store)[misalign:].view(cap, ld)[:, :v]
    sel = ops.mlm_select(hw(labels), rows, rows + 2, 8, v, cap)
    dloss = torch.randn(rows, generator=g)
    x64 = view[:slots, :v].double().clone().requires_grad_(True)
    ref_loss = F.cross_entropy(x64, labels[where], reduction="none")
    ref_loss.backward(dloss[where].double())
    return dict(logits=logits, sel=sel, labels=labels, where=where, dloss=dloss, ref_loss=ref_loss.detach(), ref_grad=x64.grad, x=view[:slots, :v],
                tie=(tie_row, lo), slots=slots, v=v)


def _run_fwd(c):
    sel = c["sel"]
    lse = ops.mlm_loss_fwd(c["logits"], sel)
    loss, pred = sel.loss_rows.cpu(), sel.pred_rows.cpu()
    labelled = torch.zeros(loss.numel(), dtype=torch.bool)
    labelled[c["where"]] = True
    assert (loss[~labelled] == 0).all() and (pred[~labelled] == IGN).all()                # padding slots write nothing
    assert torch.equal(pred[c["where"]], c["x"].double().argmax(1))
    assert pred[c["where"][c["tie"][0]]].item() == c["tie"][1]                            # the lower index of the tie
    return lse, loss[c["where"]]


def _bf16_ulps(a, b):
    """distance in bf16 steps between two bf16 tensors (sign-magnitude -> monotone integers)"""
    def key(t):
        i = t.view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("slots,v,ld,misalign", [(1, 7, 8, 0), (5, 200, 200, 0), (5, 200, 204, 0), (5, 200, 203, 1)])
def test_loss_fwd_bwd_small(hw, slots, v, ld, misalign):
    """tolerances of tests/test_kernels_misc.py for cb_cross_entropy; (5, 200, 203, 1): row starts off the 16-byte grid (scalar path)"""
    c = _loss_case(hw, slots, v, ld, seed=slots + ld, misalign=misalign)
    lse, loss = _run_fwd(c)
    torch.testing.assert_close(loss.double(), c["ref_loss"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse.cpu()[:slots].double(), torch.logsumexp(c["x"].double(), 1), rtol=1e-5, atol=1e-5)
    d32 = ops.mlm_loss_bwd(c["logits"], lse, c["sel"], hw(c["dloss"]), torch.float32)
    assert d32.shape == (slots + 1, v) and d32.dtype == torch.float32
    torch.testing.assert_close(d32.cpu()[:slots].double(), c["ref_grad"], rtol=1e-5, atol=1e-6)
    assert (d32.cpu()[slots] == 0).all()                                                  # the padding slot: zeros over the whole row
    _check_bf16(hw, c, lse, d32)


def _check_bf16(hw, c, lse, d32):
    slots = c["slots"]
    d16 = ops.mlm_loss_bwd(c["logits"], lse, c["sel"], hw(c["dloss"]), torch.bfloat16)
    assert d16.dtype == torch.bfloat16 and d16.stride(0) % 8 == 0
    assert torch.equal(d16.cpu(), d32.cpu().bfloat16())                                   # fp32 arithmetic, rounded once
    assert (d16.cpu()[slots] == 0).all()
    # ... and against the float64 reference rounded fp32 -> bf16: one bf16 step on at most 0.1 % of the elements (exp's last ulps)
    ulps = _bf16_ulps(d16.cpu()[:slots], c["ref_grad"].float().bfloat16())
    assert ulps.max().item() <= 1 and (ulps > 0).sum().item() <= 1e-3 * ulps.numel(), (ulps.max().item(), (ulps > 0).sum().item())


def test_loss_fwd_bwd_vocab(hw):
    """(3, 30522, 30524): no project tolerance exists at this width, so the bound is the parent kernel's own error: cb_cross_entropy (one
    wave per row, three passes) on the same data against the same float64 reference, times 2 -- the order of the additions is all that
    differs.  Measured max |error| (loss / gradient), new kernels vs cb_cross_entropy:
      host emulator  loss 1.011e-06 vs 1.011e-06    gradient 1.043e-07 vs 1.341e-07
      MI355X         loss 8.966e-07 vs 8.966e-07    gradient 7.448e-08 vs 1.341e-07"""
    slots, v, ld = 3, 30522, 30524
    c = _loss_case(hw, slots, v, ld, seed=11)
    lse, loss = _run_fwd(c)
    dense = hw(c["x"].contiguous())
    lab, dl = hw(c["labels"][c["where"]]), hw(c["dloss"][c["where"]])
    p_loss, p_grad = ops.cross_entropy(dense, lab, dloss=dl, want_grad=True)
    d32 = ops.mlm_loss_bwd(c["logits"], lse, c["sel"], hw(c["dloss"]), torch.float32)
    e_loss, e_grad = (loss.double() - c["ref_loss"]).abs().max().item(), (d32.cpu()[:slots].double() - c["ref_grad"]).abs().max().item()
    b_loss, b_grad = (p_loss.cpu().double() - c["ref_loss"]).abs().max().item(), (p_grad.cpu().double() - c["ref_grad"]).abs().max().item()
    print(f"\n[{hw.name}] V={v} max error: loss {e_loss:.3e} (cb_cross_entropy {b_loss:.3e}), gradient {e_grad:.3e} (cb_cross_entropy {b_grad:.3e})")
    assert e_loss <= 2 * b_loss and e_grad <= 2 * b_grad
    assert (d32.cpu()[slots] == 0).all()
    _check_bf16(hw, c, lse, d32)


@pytest.mark.gpu
def test_select_and_loss_replay_from_one_graph():
    """No host dependence on the count: select + loss forward + loss backward captured ONCE, replayed on label tensors with 2 and with 9
    labelled rows copied into the captured buffer -- each replay equals its eager run."""
    dev = torch.device("cuda", 0)
    lt, l, d, v, cap = 7, 11, 16, 200, 64
    rows = 3 * lt
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(cap, v, generator=g) * 3).to(dev)
    dloss = torch.randn(rows, generator=g).to(dev)

    def labels_with(n, seed):
        gg = torch.Generator().manual_seed(seed)
        lab = torch.full((rows,), IGN, dtype=torch.int64)
        lab[torch.randperm(rows, generator=gg)[:n]] = torch.randint(0, v, (n,), generator=gg)
        return lab

    def run(lab, counts):
        sel = ops.mlm_select(lab, lt, l, d, v, cap, counts=counts)
        lse = ops.mlm_loss_fwd(logits, sel)
        return sel, ops.mlm_loss_bwd(logits, lse, sel, dloss, torch.bfloat16)

    buf, counts = labels_with(5, 1).to(dev), torch.zeros(2, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(buf, counts)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sel, dl = run(buf, counts)
    for n, seed in ((2, 7), (9, 8)):
        lab = labels_with(n, seed).to(dev)
        buf.copy_(lab)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in (sel.loss_rows, sel.pred_rows, sel.slot_row, sel.counts, dl)]
        e_sel, e_dl = run(lab, torch.zeros(2, dtype=torch.int64, device=dev))
        torch.cuda.synchronize()
        assert got[3].tolist() == [n, 0]
        for a, b in zip(got, (e_sel.loss_rows, e_sel.pred_rows, e_sel.slot_row, e_sel.counts, e_dl)):
            assert torch.equal(a, b)
        assert (got[1] != IGN).sum().item() == n
