"""The tail form of a bottleneck block (clipbert_amd/modeling/cnn.py: _tail_form) and the residual row map it needs (cb_gemm_desc.res_rowmap).

An identity-shortcut block followed by a stride-2 block (cin 256, mid 64, cout 256; next mid 128, cout 512; n = 2): the second block reads
the first one's output at the even pixels only, so the first block runs conv2 / conv3 on the quarter map.  Tail form against today's form:
the forward of the second block comes out BIT-EQUAL (asserted: every value that is read is the same sum in the same order), d(input) and
every weight gradient agree with each other within the bound of the convolution gradients of tests/test_kernels_gemm.py, and every
launch of both backwards meets that bound against plain fp32 PyTorch on its own operands (_LaunchOracle says why launch by launch).
A 9x9 map cannot take the tail form and must run today's launches.

Recorded (host emulator and MI355X): d(input) comes out bit-equal too; the weight gradients of the tail block's conv2 / conv3 differ
from today's by ~1e-5 of values up to 200 (their pixel reduction is a quarter as long, so the fp32 partial sums group differently).

Every case runs on the host lane-level emulator build (CPU suite) and, marked `gpu`, through the real library."""
import pytest
import torch
import torch.nn.functional as F

from clipbert_amd import ops
from clipbert_amd.modeling import cnn as C
from clipbert_amd.modeling.modules import BottleneckBlock
from clipbert_amd.modeling.runtime import Runtime, even_pixel_index, even_pixel_rows

BF, F32 = torch.bfloat16, torch.float32


def tol(dt):
    return dict(rtol=2e-2, atol=2e-2) if dt == BF else dict(rtol=1e-4, atol=1e-4)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


class _Bank:
    """what the convolution launches of modeling/cnn.py ask of a ParamBank: compute-dtype KRSC weights and fp32 gradient images"""
    def __init__(self, convs, dt, dev):
        self.w = {id(c.weight): c.weight.detach().permute(0, 2, 3, 1).contiguous().to(dt).to(dev) for c in convs}
        self.g = {k: torch.zeros(v.shape[0], v[0].numel(), dtype=F32, device=dev) for k, v in self.w.items()}

    def compute(self, p):
        return self.w[id(p)]

    def grad_image(self, p):
        return self.g[id(p)]

    def is_trainable(self, p):
        return True

    def take_fresh_param(self, p):
        return False                                     # (zeroed buffers, accumulated into)

    def fold_invalidate(self):
        pass


def _blocks(seed=3):
    torch.manual_seed(seed)
    b1, b2 = BottleneckBlock(256, 64, 256, 1), BottleneckBlock(256, 128, 512, 2)
    convs = [b1.conv1, b1.conv2, b1.conv3, b2.shortcut, b2.conv1, b2.conv2, b2.conv3]
    for i, c in enumerate(convs):                        # FrozenBN with non-trivial statistics
        c.norm.weight.copy_(0.5 + torch.rand(c.cout))
        c.norm.bias.copy_(torch.randn(c.cout) * 0.2)
        c.norm.running_mean.copy_(torch.randn(c.cout) * 0.1)
        c.norm.running_var.copy_(0.5 + torch.rand(c.cout))
    return b1, b2, convs


def _oracle_forward(b1, b2, convs, x_nhwc, dt):
    """the two blocks in plain fp32 PyTorch on the rounded input and weights, every stored activation rounded where it is stored"""
    rd = lambda t: t.to(dt).float()                       # noqa: E731

    def fwd(c, t, relu=False):
        s, sh = (u.cpu().view(1, -1, 1, 1) for u in c.scale_shift())
        y = F.conv2d(t, c.weight.detach().to(dt).float(), None, c.stride, c.pad) * s + sh
        return F.relu(y) if relu else y

    x = x_nhwc.float().permute(0, 3, 1, 2).contiguous()
    o1 = rd(F.relu(fwd(b1.conv3, rd(fwd(b1.conv2, rd(fwd(b1.conv1, x, True)), True))) + x))
    o2 = rd(F.relu(fwd(b2.conv3, rd(fwd(b2.conv2, rd(fwd(b2.conv1, o1, True)), True))) + rd(fwd(b2.shortcut, o1))))
    return o2.permute(0, 2, 3, 1)


class _LaunchOracle:
    """Holds EVERY launch of a backward to plain fp32 PyTorch (torch.nn.grad) on that launch's own operands, with the bound of the
    convolution gradients of tests/test_kernels_gemm.py.  The bound is a single launch's: a chain of nine launches compared end to end
    against an fp32 chain misses it for today's launches too (measured here: one output of 25600 lies 5e-6 from zero, its ReLU mask flips
    between two fp32 summation orders and moves a 3x3 patch of d(input) by 0.2; one bf16 activation rounds the other way and moves a
    weight-gradient element by 0.1) -- so every launch is checked where it runs, on what it was given."""
    def __init__(self, dt):
        self.dt, self.dw, self.launches = dt, {}, 0
        self._d, self._w = C._conv_dgrad, C._conv_wgrad

    @staticmethod
    def _nchw(t):
        return t.float().cpu().permute(0, 3, 1, 2).contiguous()

    def _weight(self, rt, conv):
        w = rt.bank.compute(conv.weight).float().cpu()
        return w.view(conv.cout, conv.k, conv.k, conv.cin).permute(0, 3, 1, 2).contiguous()

    def dgrad(self, rt, g, conv, in_shape, scale=None, mask=None, residual=None, out=None, accumulate=False, fuse=None, res_rowmap=None):
        from torch.nn.grad import conv2d_input
        n, h, w, cin = in_shape
        before = out.float().cpu().clone() if accumulate else None
        got = self._d(rt, g, conv, in_shape, scale=scale, mask=mask, residual=residual, out=out, accumulate=accumulate, fuse=fuse, res_rowmap=res_rowmap)
        want = conv2d_input((n, cin, h, w), self._weight(rt, conv), self._nchw(g), conv.stride, conv.pad).permute(0, 2, 3, 1)
        if accumulate:
            want = want + before
        if residual is not None:
            r = residual.float().cpu().view(-1, cin)
            if res_rowmap is not None:
                m = res_rowmap.cpu().long()
                r = torch.where((m >= 0).view(-1, 1), r[m.clamp_min(0)], torch.zeros(n * h * w, cin))
            want = want + r.view(n, h, w, cin)
        f = lambda t: t.float().cpu()                     # noqa: E731
        if fuse is not None:
            y, s_a, s_b = fuse
            t = torch.where(f(y).view(n, h, w, cin) > 0, want, torch.zeros_like(want))
            torch.testing.assert_close(f(got[0]), t * f(s_a), **tol(self.dt))
            torch.testing.assert_close(f(got[1]), t * f(s_b) if s_b is not None else t, **tol(self.dt))
        else:
            if scale is not None:
                want = want * f(scale)
            if mask is not None:
                want = torch.where(f(mask).view(n, h, w, cin) > 0, want, torch.zeros_like(want))
            torch.testing.assert_close(f(got), want, **tol(self.dt))
        self.launches += 1
        return got

    def wgrad(self, rt, g, x, conv, pending=None):
        from torch.nn.grad import conv2d_weight
        want = conv2d_weight(self._nchw(x), (conv.cout, conv.cin, conv.k, conv.k), self._nchw(g), conv.stride, conv.pad)
        self.dw[id(conv.weight)] = want.permute(0, 2, 3, 1).reshape(conv.cout, -1)          # (compared once the grouped launch has run)
        return self._w(rt, g, x, conv, pending)


def _run(hw, dt, b1, b2, convs, x, dy, tail, monkeypatch):
    rt = Runtime()
    rt.dtype = dt
    rt.bank = _Bank(convs, dt, hw.dev)
    out, saved = C.blocks_forward(rt, hw(x), [[b1], [b2]], save=True, tail=tail)
    # ReLU x FrozenBN backward of the last block, as the launch that produces d(out) would do it
    t = torch.where(out.float() > 0, hw(dy).float(), torch.zeros_like(out.float()))
    g3 = (t * b2.conv3.scale_shift()[0]).to(dt)
    sec = (t * b2.shortcut.scale_shift()[0]).to(dt)
    pend, dx = [], []

    def flush():
        ops.gemm_group(pend, g3)
        pend.clear()

    chk = _LaunchOracle(dt)
    with monkeypatch.context() as mp:
        mp.setattr(C, "_conv_dgrad", chk.dgrad)
        mp.setattr(C, "_conv_wgrad", chk.wgrad)
        for _ in C.blocks_backward(rt, saved, g3, sec, {}, flush, pend, dx_out=dx):
            pass
    assert chk.launches == 7 and len(chk.dw) == 7        # (data gradients: conv3, conv2 of both blocks; conv1, shortcut of the second; conv1 of the first)
    dw = {id(c): rt.bank.g[id(c.weight)] for c in convs}
    for c in convs:
        torch.testing.assert_close(dw[id(c)].cpu(), chk.dw[id(c.weight)], **tol(dt))
    return out, saved, dx[0], dw


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("H,W", [(8, 12), (12, 12), (9, 9)])
def test_tail_form_against_todays_form_and_the_oracle(hw, monkeypatch, H, W, dt):
    n = 2
    b1, b2, convs = _blocks()
    for b in (b1, b2):
        b.to(hw.dev)
    x = rnd(n, H, W, 256, seed=1).relu().to(dt)          # (a block input is a ReLU output)
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = rnd(n, oh, ow, 512, seed=2).to(dt)
    # (both runs hold each of their backward launches to the oracle: _LaunchOracle)
    out_t, saved_t, dx_t, dw_t = _run(hw, dt, b1, b2, convs, x, dy, True, monkeypatch)
    out_o, saved_o, dx_o, dw_o = _run(hw, dt, b1, b2, convs, x, dy, False, monkeypatch)
    even = H % 2 == 0 and W % 2 == 0
    assert [(r[5], r[6]) for r in saved_t] == ([(True, False), (False, True)] if even else [(False, False), (False, False)])
    assert [(r[5], r[6]) for r in saved_o] == [(False, False), (False, False)]
    if even:                                             # the quarter map is what the tail block keeps
        assert saved_t[0][3].shape == (n, H // 2, W // 2, 64) and saved_t[0][4].shape == (n, H // 2, W // 2, 256)
        assert torch.equal(saved_t[0][4].cpu().view(-1, 256), saved_o[0][4].cpu().view(-1, 256)[even_pixel_rows(n, H, W)])
    assert torch.equal(out_t, out_o)                     # forward of the second block: bit-equal
    for b in (b1, b2):
        b.cpu()
    f = lambda t: t.float().cpu()                         # noqa: E731
    ref_out = _oracle_forward(b1, b2, convs, x, dt)
    print(f"[block tail {hw.name}] {H}x{W} {dt}: out vs oracle {float((f(out_t) - ref_out).abs().max()):.3e}; d(input) tail vs today "
          f"{float((f(dx_t) - f(dx_o)).abs().max()):.3e}, bit-equal {torch.equal(dx_t, dx_o)}; dW tail vs today "
          + " ".join(f"{float((f(dw_t[id(c)]) - f(dw_o[id(c)])).abs().max()):.2e}" for c in convs))
    torch.testing.assert_close(f(out_t), ref_out, **tol(dt))
    torch.testing.assert_close(f(dx_t), f(dx_o), **tol(dt))
    for c in convs:
        torch.testing.assert_close(f(dw_t[id(c)]), f(dw_o[id(c)]), **tol(dt))


def _maps(n, H, W, kind):
    """(M, residual rows, map): compact row -> row of the whole map with some rows switched off, or row of the whole map -> compact row / -1"""
    if kind == "gather":
        m = even_pixel_rows(n, H, W).clone()
        m[::5] = -1
        return m.numel(), n * H * W, m
    return n * H * W, n * (H // 2) * (W // 2), even_pixel_index(n, H, W)


@pytest.mark.parametrize("dt,tile", [(BF, 2), (BF, 3), (BF, 1), (BF, 4), (F32, 2)])
@pytest.mark.parametrize("kind", ["gather", "scatter"])
@pytest.mark.parametrize("N,extra_act", [(72, False), (72, True), (36, False), (37, False)])
def test_residual_row_map_forward(hw, kind, N, extra_act, dt, tile):
    """FrozenBN + residual + ReLU with the residual read through its own row map, -1 rows included: the specialised body (72 columns), the
    generic row-contiguous epilogue (an activation the listed combination does not have), the 4-wide and the per-element epilogues"""
    n, H, W, K = 2, 8, 12, 64
    M, rrows, rmap = _maps(n, H, W, kind)
    x, w = rnd(M, K, seed=1).to(dt), rnd(N, K, seed=2, scale=0.2).to(dt)
    res = rnd(rrows, N, seed=3).to(dt)
    scale, shift = rnd(N, seed=4).abs() + 0.5, rnd(N, seed=5)
    out = torch.empty(M, N, dtype=dt, device=hw.dev)
    ops.gemm(hw(x), hw(w), M, N, K, out=out, scale=hw(scale), shift=hw(shift), act=ops.ACT_RELU if extra_act else ops.ACT_NONE, residual=hw(res),
             res_rowmap=hw(rmap.int()), relu_after=True, tile=tile)
    v = x.float() @ w.float().t() * scale + shift
    if extra_act:
        v = F.relu(v)
    gathered = torch.where((rmap >= 0).view(-1, 1), res.float()[rmap.clamp_min(0)], torch.zeros(M, N))
    torch.testing.assert_close(out.float().cpu(), F.relu(v + gathered), **tol(dt))
    # the same call with the residual gathered beforehand: the same bits
    out2 = torch.empty(M, N, dtype=dt, device=hw.dev)
    ops.gemm(hw(x), hw(w), M, N, K, out=out2, scale=hw(scale), shift=hw(shift), act=ops.ACT_RELU if extra_act else ops.ACT_NONE,
             residual=hw(gathered.to(dt)), relu_after=True, tile=tile)
    assert torch.equal(out, out2)


@pytest.mark.parametrize("dt,tile", [(BF, 2), (BF, 3), (BF, 1), (BF, 4), (F32, 2)])
@pytest.mark.parametrize("kind", ["gather", "scatter"])
@pytest.mark.parametrize("N", [72, 36])
def test_residual_row_map_relu_bwd(hw, kind, N, dt, tile):
    """the data-gradient launch that also does the consumer's ReLU x FrozenBN backward, its residual (the identity-shortcut gradient) through
    a row map: with the epilogue operands prefetched (64x64 / 128x64 tiles) and requested by the body itself (128x128)"""
    n, H, W, K = 2, 8, 12, 40
    M, rrows, rmap = _maps(n, H, W, kind)
    g, w = rnd(M, K, seed=1).to(dt), rnd(K, N, seed=2, scale=0.2).to(dt)
    y, res = rnd(M, N, seed=3).to(dt), rnd(rrows, N, seed=4).to(dt)
    sa = rnd(N, seed=5).abs() + 0.5
    c, c2 = torch.empty(M, N, dtype=dt, device=hw.dev), torch.empty(M, N, dtype=dt, device=hw.dev)
    ops.gemm(hw(g), hw(w), M, N, K, out=c, b_mode=ops.KROW, ldb=N, tile=tile, residual=hw(res), res_rowmap=hw(rmap.int()), mask=hw(y), relu_bwd=True,
             post_scale=hw(sa), out2=c2)
    gathered = torch.where((rmap >= 0).view(-1, 1), res.float()[rmap.clamp_min(0)], torch.zeros(M, N))
    t = torch.where(y.float() > 0, g.float() @ w.float() + gathered, torch.zeros(M, N))
    torch.testing.assert_close(c2.float().cpu(), t, **tol(dt))
    torch.testing.assert_close(c.float().cpu(), t * sa, **tol(dt))
    d, d2 = torch.empty_like(c), torch.empty_like(c2)
    ops.gemm(hw(g), hw(w), M, N, K, out=d, b_mode=ops.KROW, ldb=N, tile=tile, residual=hw(gathered.to(dt)), mask=hw(y), relu_bwd=True,
             post_scale=hw(sa), out2=d2)
    assert torch.equal(c, d) and torch.equal(c2, d2)


def test_row_map_is_refused_where_it_cannot_run(hw):
    M, N, K = 96, 72, 64
    x, w, res = hw(rnd(M, K, seed=1).to(BF)), hw(rnd(N, K, seed=2).to(BF)), hw(rnd(M, N, seed=3).to(BF))
    out = torch.empty(M, N, dtype=BF, device=hw.dev)
    rmap = hw(torch.arange(M).int())
    for asked in (0, 5, 6, 7):                             # the 8-wave tiles have no row-map bodies: the call falls to the 4-wave kernels
        assert ops.gemm_plan(x, w, M, N, K, out=out, residual=res, res_rowmap=rmap, tile=asked)[0] in (1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="tile 8"):
        ops.gemm(x, w, M, N, K, out=out, residual=res, res_rowmap=rmap, tile=8)
