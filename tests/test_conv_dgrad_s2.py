"""Data gradient of a 3x3 stride-2 pad-1 convolution in one launch, by parity classes (cb_gemm_desc.dgrad_s2), and the stride-2 gather
forward it belongs to.  Oracle: plain PyTorch fp32 on the (bf16-rounded) inputs, with the bound of the 3x3 data-gradient cases of
tests/test_kernels_gemm.py.  Second yardstick: today's stride-1 flipped-tap launch fed the zero-inserted gradient -- the same sums with
the zero products left in; the two must agree to 1 bf16 ulp.

Recorded: on the MI355X the two launches come out BIT-EQUAL on every case of this file.  On the host emulator they are bit-equal at 64
channels and in the fp32 mode; the plain bf16 case at 72 channels differs by exactly 1 bf16 ulp in a few elements (a 64-deep K tile then
straddles two taps, so the 32 products of one MFMA are grouped with different neighbours and the emulator adds them in another order).
Every product the class form drops is an exact zero, and the taps that remain are added in the same order.

Every case runs on the host lane-level emulator build (CPU suite) and, marked `gpu`, through the real library."""
import pytest
import torch
import torch.nn.functional as F

from clipbert_amd import ops
from clipbert_amd.modeling.runtime import even_pixel_rows, parity_class_rows

BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(2, 8, 12, 64),       # 48 rows per class: partial tiles only
          (3, 12, 12, 64),      # 108 rows per class: one full 64-row tile and a partial one
          (3, 12, 12, 72)]      # K tail (72 channels per tap against 64-deep K tiles), 16-byte rows
# the 4-wave tiles (2 = 64x64, 3 = 128x64, 1 = 128x128) in bf16; the fp32 parity mode has the 64x64 tile only
KINDS = [(BF, 2), (BF, 3), (BF, 1), (F32, 2)]


def tol(dt):
    return dict(rtol=2e-2, atol=2e-2) if dt == BF else dict(rtol=1e-4, atol=1e-4)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def within_one_bf16_ulp(a, b):
    """largest distance of a from b in units of the bf16 spacing at max(|a|, |b|) (2^-7 of its binade); <= 1 passes"""
    a, b = a.double(), b.double()
    big = torch.maximum(a.abs(), b.abs()).clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(big)) - 7)
    return float(((a - b).abs() / ulp).max())


def problem(hw, dt, n, H, W, C):
    """g: gradient of the (n, H/2, W/2, C) output; w: (C, C, 3, 3); the two kernels' inputs on the backend"""
    g = rnd(n, C, H // 2, W // 2, seed=1).to(dt)
    w = rnd(C, C, 3, 3, seed=2, scale=0.1).to(dt)
    gh = hw(g.permute(0, 2, 3, 1).contiguous())
    wk = hw(w.permute(0, 2, 3, 1).contiguous())          # KRSC
    ref = F.conv_transpose2d(g.float(), w.float(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1).contiguous()     # (n, H, W, C)
    return gh, wk, ref


def dgrad_classes(hw, gh, wk, n, H, W, C, tile, **epi):
    oh, ow = H // 2, W // 2
    tab = ops.build_pixel_table(n, oh, ow, 1, 0, oh * ow * C, ow * C, C, gh.device)
    out = torch.full((n * H * W, C), float("nan"), dtype=gh.dtype, device=hw.dev)
    ops.gemm(gh, wk, n * H * W, C, 9 * C, out=out, a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, b_mode=ops.KROW_TAPS, ldb=9 * C, R=3, S=3, Cin=C,
             H=oh, W=ow, sH=ow * C, sW=C, dgrad_s2=True, c_rowmap=hw(parity_class_rows(n, H, W).int()), tile=tile, **epi)
    return out


def dgrad_zero_inserted(hw, gh, wk, n, H, W, C, tile, **epi):
    """today's form: the stride-1 transposed convolution (flipped taps, pad 1) over the gradient with zeros at the odd pixels"""
    full = torch.zeros(n * H * W, C, dtype=gh.dtype, device=hw.dev)
    full[hw(even_pixel_rows(n, H, W))] = gh.view(-1, C)
    tab = ops.build_pixel_table(n, H, W, 1, 1, H * W * C, W * C, C, gh.device)
    out = torch.empty(n * H * W, C, dtype=gh.dtype, device=hw.dev)
    ops.gemm(full, wk, n * H * W, C, 9 * C, out=out, a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, b_mode=ops.KROW_TAPS, ldb=9 * C, R=3, S=3, Cin=C,
             H=H, W=W, sH=W * C, sW=C, flip_taps=True, tile=tile, **epi)
    return out


@pytest.mark.parametrize("epilogue", ["plain", "scale+mask"])
@pytest.mark.parametrize("dt,tile", KINDS)
@pytest.mark.parametrize("n,H,W,C", SHAPES)
def test_dgrad_s2_against_oracle_and_zero_inserted_form(hw, n, H, W, C, dt, tile, epilogue):
    gh, wk, ref = problem(hw, dt, n, H, W, C)
    epi = {}
    if epilogue != "plain":
        mask = rnd(n * H * W, C, seed=3).to(dt)
        scale = rnd(C, seed=4).abs() + 0.5
        epi = dict(scale=hw(scale), mask=hw(mask))
        ref = torch.where(mask.float().view(n, H, W, C) > 0, ref * scale, torch.zeros_like(ref))
    got = dgrad_classes(hw, gh, wk, n, H, W, C, tile, **epi).float().cpu().view(n, H, W, C)
    old = dgrad_zero_inserted(hw, gh, wk, n, H, W, C, tile, **epi).float().cpu().view(n, H, W, C)
    ulps = within_one_bf16_ulp(got, old)
    print(f"[dgrad_s2 {hw.name}] n={n} {H}x{W} C={C} {dt} tile {tile} {epilogue}: max |err| vs oracle {float((got - ref).abs().max()):.3e}, "
          f"vs zero-inserted form {ulps:.3f} bf16 ulp, bit-equal {torch.equal(got, old)}")
    assert not torch.isnan(got).any()                  # every input pixel is written by exactly one class
    # the borders, where windows leave the gradient map (y = H - 1 reaches row H / 2 of g) and where the padding taps fall away
    torch.testing.assert_close(got[:, 0], ref[:, 0], **tol(dt))
    torch.testing.assert_close(got[:, -1], ref[:, -1], **tol(dt))
    torch.testing.assert_close(got[:, :, 0], ref[:, :, 0], **tol(dt))
    torch.testing.assert_close(got[:, :, -1], ref[:, :, -1], **tol(dt))
    torch.testing.assert_close(got, ref, **tol(dt))
    assert ulps <= 1.0


@pytest.mark.parametrize("dt,tile", KINDS)
@pytest.mark.parametrize("n,H,W,C", SHAPES)
def test_gather_forward_3x3_stride2(hw, n, H, W, C, dt, tile):
    """the forward that goes with it: the pixel table's stride at k = 3, s = 2 (the model ran it at k = 7 and k = 1 only)"""
    x = rnd(n, C, H, W, seed=5).to(dt)
    w = rnd(C, C, 3, 3, seed=2, scale=0.1).to(dt)
    scale, shift = rnd(C, seed=6).abs() + 0.5, rnd(C, seed=7)
    xh, wk = hw(x.permute(0, 2, 3, 1).contiguous()), hw(w.permute(0, 2, 3, 1).contiguous())
    oh, ow = H // 2, W // 2
    tab = ops.build_pixel_table(n, oh, ow, 2, 1, H * W * C, W * C, C, xh.device)
    y = torch.empty(n * oh * ow, C, dtype=dt, device=hw.dev)
    ops.gemm(xh, wk, n * oh * ow, C, 9 * C, out=y, a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, ldb=9 * C, R=3, S=3, Cin=C, H=H, W=W, sH=W * C, sW=C,
             scale=hw(scale), shift=hw(shift), act=ops.ACT_RELU, tile=tile)
    ref = F.relu(F.conv2d(x.float(), w.float(), None, 2, 1) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    torch.testing.assert_close(y.float().cpu().view(n, oh, ow, C), ref, **tol(dt))
    # ... and it is the stride-1 convolution at the even pixels, bit for bit (same windows, same order)
    tab1 = ops.build_pixel_table(n, H, W, 1, 1, H * W * C, W * C, C, xh.device)
    y1 = torch.empty(n * H * W, C, dtype=dt, device=hw.dev)
    ops.gemm(xh, wk, n * H * W, C, 9 * C, out=y1, a_mode=ops.ROWK_GATHER, a_tab=tab1, lda=0, ldb=9 * C, R=3, S=3, Cin=C, H=H, W=W, sH=W * C, sW=C,
             scale=hw(scale), shift=hw(shift), act=ops.ACT_RELU, tile=tile)
    assert torch.equal(y.cpu(), y1.cpu()[even_pixel_rows(n, H, W)])


def test_library_chooses_a_4wave_tile_and_refuses_malformed_calls(hw):
    n, H, W, C = 2, 8, 12, 64
    gh, wk, _ = problem(hw, BF, n, H, W, C)
    oh, ow = H // 2, W // 2
    tab = ops.build_pixel_table(n, oh, ow, 1, 0, oh * ow * C, ow * C, C, gh.device)
    out = torch.empty(n * H * W, C, dtype=BF, device=hw.dev)
    kw = dict(out=out, a_mode=ops.ROWK_GATHER, a_tab=tab, lda=0, b_mode=ops.KROW_TAPS, ldb=9 * C, R=3, S=3, Cin=C, H=oh, W=ow, sH=ow * C, sW=C,
              dgrad_s2=True, c_rowmap=hw(parity_class_rows(n, H, W).int()))
    for asked in (0, 5, 7):                                # (an 8-wave tile asked for falls to the 4-wave kernels, as for every form they do not cover)
        assert ops.gemm_plan(gh, wk, n * H * W, C, 9 * C, tile=asked, **kw)[0] in (1, 2, 3, 4)
    with pytest.raises(RuntimeError, match="dgrad_s2"):
        ops.gemm(gh, wk, n * H * W, C, 9 * C, **dict(kw, c_rowmap=None))
    with pytest.raises(RuntimeError, match="dgrad_s2"):
        ops.gemm(gh, wk, n * H * W, C, 9 * C, **dict(kw, ldb=C))
