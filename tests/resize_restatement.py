"""The input transform of the reference restated in a dozen lines of torch -- the yardstick of tests/test_resize_pack.py and
tests/test_raw_frames.py wherever the reference tree is absent (the GPU box).  Per video: ``ImageResize(S, "bilinear")`` on the
FLOAT frames (F.interpolate, align_corners=False, to get_resize_size's size), ``ImagePad(S, S)`` (zeros to the right and below),
src/datasets/dataset_base.py:270-273; per batch ``ImageNorm`` ((x - mean) / std, src/datasets/data_utils.py:256-276).
test_resize_pack.py::test_restatement_equals_reference_live pins every function here to the reference's classes bit for bit.
Helper module: no tests in here."""
import torch
import torch.nn.functional as F

# (T, h, w) of a video -> S: portrait, landscape, square, upscaling (100 x 180 -> 224), a truncating ratio (333 x 500 -> 768: 511)
PIN_CASES = [((2, 240, 320), 224), ((1, 360, 640), 224), ((2, 100, 180), 224), ((1, 480, 360), 448), ((1, 720, 1280), 448),
             ((1, 333, 500), 768), ((2, 96, 96), 64), ((1, 64, 64), 64), ((1, 200, 41), 64)]


def resize_size(h, w, max_size):
    """get_resize_size (data_utils.py:167-199) for a tensor of height h and width w"""
    if h >= w:
        return int(max_size), int(max_size * (w * 1. / h))
    return int(max_size * (h * 1. / w)), int(max_size)


def resize_pad(frames_u8: torch.Tensor, S: int) -> torch.Tensor:
    """(T, 3, h, w) uint8 -> (T, 3, S, S) fp32 in 0..255: what _load_video returns for these frames"""
    x = frames_u8.float()
    nh, nw = resize_size(x.shape[-2], x.shape[-1], S)
    x = F.interpolate(x, size=(nh, nw), mode="bilinear", align_corners=False)
    return F.pad(x, (0, S - nw, 0, S - nh), "constant", 0)


def image_norm(x: torch.Tensor, mean, std) -> torch.Tensor:
    """ImageNorm on a (..., 3, H, W) fp32 batch of 0..255 pixels with 0..255 statistics"""
    m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    return (x - m) / s


def dense_batch(videos, S: int) -> torch.Tensor:
    """planar uint8 videos (T, 3, h, w), any h x w each -> the collated (B, T, 3, S, S) fp32 batch before ImageNorm"""
    return torch.stack([resize_pad(v, S) for v in videos])


def packed_reference(padded: torch.Tensor, new_sizes, mean, std, pad: int = 3, extra_w: int = 0):
    """The packed stem image the library must produce for ``padded`` (N, 3, S, S) (resize_pad's output): BGR0, ``pad`` zeros around,
    normalised in the LIBRARY's convention (v - mean) * (1 / std) in fp32 (cb_stem_pack's; equal to ImageNorm's division up to one
    rounding, and identical for the model's default std of 1).  Also the boolean interior mask (N, S, S) of the new_h x new_w regions."""
    n, _, S, _ = padded.shape
    m = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    istd = (1.0 / torch.tensor(std, dtype=torch.float32)).view(1, 3, 1, 1)
    normed = (padded - m) * istd
    out = torch.zeros(n, S + 2 * pad, S + 2 * pad + extra_w, 4, dtype=torch.float32)
    out[:, pad:pad + S, pad:pad + S, :3] = normed[:, [2, 1, 0]].permute(0, 2, 3, 1)
    interior = torch.zeros(n, S, S, dtype=torch.bool)
    for i, (nh, nw) in enumerate(new_sizes):
        interior[i, :nh, :nw] = True
    return out, interior


def random_video(t, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (t, 3, h, w), generator=g, dtype=torch.uint8)
