"""cb_vqa_loss_fwd / cb_vqa_loss_bwd through clipbert_amd.ops: loss row sums, arg-max, the VQA score of the arg-max and the gradient of the
sparse-answer BCE head against torch's binary_cross_entropy_with_logits on the dense targets in float64."""
import pytest
import torch
import torch.nn.functional as F

from clipbert_amd import ops
from clipbert_amd.data import vqa_dense_targets
from test_mlm_select import _bf16_ulps

SCORES = (0.3, 0.6, 0.9, 1.0)
CASES = [(1, 2, 2, 0, 1), (3, 5, 8, 0, 2), (3, 259, 259, 0, 10), (3, 1030, 1032, 0, 4), (2, 3129, 3129, 1, 10), (3, 3129, 3132, 0, 10)]


def _case(hw, rows, c, ld, misalign, k, seed=0):
    """logits (rows, c) with row stride ld behind ``misalign`` floats, pad columns +1e30; row 0: every slot valid, its first answer is the
    arg-max (+80 at column 0; -80 at column c - 1); row 1: one valid slot that is NOT the arg-max and one slot with id >= c; row 2: all
    padding with garbage scores; the last row (when there is more than one) has a two-way tie of its maximum"""
    g = torch.Generator().manual_seed(seed)
    store = torch.full((rows * ld + misalign,), 1e30)
    view = store[misalign:].view(rows, ld)
    view[:, :c] = torch.randn(rows, c, generator=g) * 3
    view[0, 0], view[0, c - 1] = 80.0, -80.0
    tie = None
    if rows > 1:
        lo, hi = (1, c - 2) if c > 3 else (0, c - 1)
        view[rows - 1, lo] = view[rows - 1, hi] = view[rows - 1, :c].max() + 1.0
        tie = (rows - 1, lo)
    ids = torch.full((rows, k), -1, dtype=torch.int32)
    scores = torch.zeros(rows, k)
    others = 1 + torch.randperm(c - 1, generator=g)[:k - 1]                                # distinct columns, none of them 0
    ids[0] = torch.cat([torch.zeros(1, dtype=torch.long), others]).to(torch.int32)
    scores[0] = torch.tensor(SCORES)[torch.randint(0, 4, (k,), generator=g)]
    if rows > 1:
        best = int(view[1, :c].argmax())
        ids[1, 0], scores[1, 0] = (best + 2) % c, 0.6
        ids[1, 1], scores[1, 1] = c + 3, 0.7                                              # id >= c: padding, its score is never used
    if rows > 2:
        ids[2, ::2], scores[2] = c, 0.5                                                   # all padding (-1 and c), garbage scores
    dloss = torch.randn(rows, generator=g)
    x = view[:, :c]
    dense = vqa_dense_targets(ids, scores, c)
    x64 = x.double().clone().requires_grad_(True)
    ref_loss = F.binary_cross_entropy_with_logits(x64, dense.double(), reduction="none").sum(1)
    ref_loss.backward(dloss.double())
    scale = F.softplus(x.double()).sum(1) + (dense.double() * x.double()).abs().sum(1)     # sum_c softplus(x_c) + sum_k |s_k x[a_k]|
    logits = hw(store)[misalign:].view(rows, ld)[:, :c]
    return dict(logits=logits, ids=hw(ids), scores=hw(scores), dloss=hw(dloss), x=x, dense=dense, ref_loss=ref_loss.detach(), ref_grad=x64.grad,
                scale=scale, tie=tie, rows=rows, c=c)


def _padded(d):
    """the whole (rows, ldd) buffer behind the (rows, C) view that vqa_loss_bwd returns"""
    return torch.as_strided(d, (d.shape[0], d.stride(0)), (d.stride(0), 1))


@pytest.mark.parametrize("rows,c,ld,misalign,k", CASES)
def test_loss_pred_score_and_gradients(hw, rows, c, ld, misalign, k):
    """Loss: |err| <= 1e-5 x (sum_c softplus(x_c) + sum_k |s_k x[a_k]|) per row -- fp32 eps 6e-8 x ~40 accumulated roundings (a per-thread
    partial of ceil(C / 256) terms, an 8-level tree, a few ulps per term) = 2.4e-6, with a 4x margin; cb_cross_entropy's rtol.  fp32 gradient:
    the bounds of test_loss_fwd_bwd_small (tests/test_mlm_select.py); bf16: rounded once from the fp32 arithmetic, one bf16 step from the
    float64 gradient on at most 0.1 % of the elements."""
    t = _case(hw, rows, c, ld, misalign, k, seed=rows + ld)
    loss, pred, score = ops.vqa_loss_fwd(t["logits"], t["ids"], t["scores"])
    assert loss.shape == pred.shape == score.shape == (rows,) and pred.dtype == torch.int64 and loss.dtype == score.dtype == torch.float32
    err = (loss.cpu().double() - t["ref_loss"]).abs()
    print(f"\n[{hw.name}] rows {rows} C {c} ld {ld}: max loss error / scale {float((err / t['scale']).max()):.3e}")
    assert (err <= 1e-5 * t["scale"]).all(), (err, t["scale"])
    want = t["x"].double().argmax(1)
    no_tie = [r for r in range(rows) if t["tie"] is None or r != t["tie"][0]]
    assert torch.equal(pred.cpu()[no_tie], want[no_tie])
    if t["tie"] is not None:
        assert pred.cpu()[t["tie"][0]].item() == t["tie"][1]                               # the lower index of the tie
    assert pred.cpu()[0].item() == 0
    want_score = t["dense"][torch.arange(rows), pred.cpu()]                                # the target at the arg-max: its annotated score or 0
    assert torch.equal(score.cpu(), want_score), (score, want_score)
    assert score.cpu()[0].item() == t["scores"].cpu()[0, 0].item() and (score.cpu()[1:] == 0).all()

    d32 = ops.vqa_loss_bwd(t["logits"], t["ids"], t["scores"], t["dloss"], torch.float32)
    assert d32.shape == (rows, c) and d32.dtype == torch.float32 and d32.stride(0) % 4 == 0
    torch.testing.assert_close(d32.cpu().double(), t["ref_grad"], rtol=1e-5, atol=1e-6)
    assert (_padded(d32).cpu()[:, c:] == 0).all()
    d16 = ops.vqa_loss_bwd(t["logits"], t["ids"], t["scores"], t["dloss"], torch.bfloat16)
    assert d16.shape == (rows, c) and d16.dtype == torch.bfloat16 and d16.stride(0) % 8 == 0
    assert torch.equal(d16.cpu(), d32.cpu().bfloat16())                                    # fp32 arithmetic, rounded once
    assert (_padded(d16).cpu()[:, c:] == 0).all()
    ulps = _bf16_ulps(d16.cpu(), t["ref_grad"].float().bfloat16())
    assert ulps.max().item() <= 1 and (ulps > 0).sum().item() <= 1e-3 * ulps.numel(), (ulps.max().item(), (ulps > 0).sum().item())


def test_duplicate_slots_add_up(hw):
    """valid slots of one row that name the same id add up, in the loss, the score of the prediction and the gradient"""
    x = torch.tensor([[0.5, 2.0, -1.0, 0.25, 1.5]])
    ids, sc = torch.tensor([[1, 3, 1]], dtype=torch.int32), torch.tensor([[0.3, 0.6, 0.3]])
    dense = torch.tensor([[0.0, 0.6, 0.0, 0.6, 0.0]])
    loss, pred, score = ops.vqa_loss_fwd(hw(x), hw(ids), hw(sc))
    want = F.binary_cross_entropy_with_logits(x.double(), dense.double(), reduction="none").sum(1)
    torch.testing.assert_close(loss.cpu().double(), want, rtol=1e-5, atol=0)
    assert pred.cpu().tolist() == [1] and score.cpu().item() == pytest.approx(0.6, abs=1e-7)
    d = ops.vqa_loss_bwd(hw(x), hw(ids), hw(sc), hw(torch.ones(1)), torch.float32)
    torch.testing.assert_close(d.cpu().double(), torch.sigmoid(x.double()) - dense.double(), rtol=1e-5, atol=1e-6)


def test_bad_shapes_fail_with_a_message_and_no_rows_is_a_no_op(hw):
    x = hw(torch.randn(3, 5))
    dl = hw(torch.ones(3))
    for k in (0, 33):
        ids, sc = hw(torch.zeros(3, k, dtype=torch.int32)), hw(torch.zeros(3, k))
        with pytest.raises(RuntimeError, match=r"cb_vqa_loss_fwd: bad shape \(rows 3, C 5, ld 5, K %d: 1\.\.32\)" % k):
            ops.vqa_loss_fwd(x, ids, sc)
        with pytest.raises(RuntimeError, match=r"cb_vqa_loss_bwd: bad shape \(rows 3, C 5, ld 5, ldd \d+, K %d: 1\.\.32\)" % k):
            ops.vqa_loss_bwd(x, ids, sc, dl, torch.float32)
    ids, sc = hw(torch.zeros(3, 2, dtype=torch.int32)), hw(torch.zeros(3, 2))
    narrow = hw(torch.randn(16)).as_strided((3, 5), (4, 1))                                # ld < C
    with pytest.raises(RuntimeError, match=r"cb_vqa_loss_fwd: bad shape \(rows 3, C 5, ld 4,"):
        ops.vqa_loss_fwd(narrow, ids, sc)
    with pytest.raises(RuntimeError, match=r"cb_vqa_loss_bwd: bad shape \(rows 3, C 5, ld 4,"):
        ops.vqa_loss_bwd(narrow, ids, sc, dl, torch.bfloat16)
    none = ops.vqa_loss_fwd(hw(torch.zeros(0, 7)), hw(torch.zeros(0, 3, dtype=torch.int32)), hw(torch.zeros(0, 3)))
    assert [tuple(t.shape) for t in none] == [(0,)] * 3 and none[1].dtype == torch.int64
    d = ops.vqa_loss_bwd(hw(torch.zeros(0, 7)), hw(torch.zeros(0, 3, dtype=torch.int32)), hw(torch.zeros(0, 3)), hw(torch.zeros(0)), torch.bfloat16)
    assert d.shape == (0, 7) and d.dtype == torch.bfloat16


def test_abi_version_names_the_vqa_entry_points():
    from clipbert_amd import _lib
    assert _lib.get().cb_version() >= 13 and {"cb_vqa_loss_fwd", "cb_vqa_loss_bwd"} <= set(_lib.EXPORTED_SYMBOLS)


@pytest.mark.gpu
def test_loss_forward_and_backward_replay_from_one_graph():
    """Fixed-shape answer tables: forward + backward captured ONCE, replayed on two other tables (3 and 9 answers per question) copied into
    the captured buffers -- each replay equals its eager run."""
    dev = torch.device("cuda", 0)
    rows, c, k = 4, 3129, 10
    g = torch.Generator().manual_seed(3)
    logits = torch.empty(rows, 3132, device=dev)[:, :c]
    logits.copy_((torch.randn(rows, c, generator=g) * 3).to(dev))
    dloss = torch.randn(rows, generator=g).to(dev)

    def tables(n, seed):
        gg = torch.Generator().manual_seed(seed)
        ids = torch.full((rows, k), -1, dtype=torch.int32)
        sc = torch.zeros(rows, k)
        for r in range(rows):
            ids[r, :n] = torch.randperm(c, generator=gg)[:n].to(torch.int32)
            sc[r, :n] = torch.tensor(SCORES)[torch.randint(0, 4, (n,), generator=gg)]
        return ids.to(dev), sc.to(dev)

    def run(ids, sc):
        return ops.vqa_loss_fwd(logits, ids, sc) + (ops.vqa_loss_bwd(logits, ids, sc, dloss, torch.bfloat16),)

    ids_buf, sc_buf = tables(5, 1)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(ids_buf, sc_buf)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run(ids_buf, sc_buf)
    seen = []
    for n, seed in ((3, 7), (9, 8)):
        ids, sc = tables(n, seed)
        ids_buf.copy_(ids)
        sc_buf.copy_(sc)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        want = run(ids, sc)
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        seen.append(got[0])
    assert not torch.equal(seen[0], seen[1])                                               # the two replays saw different targets
