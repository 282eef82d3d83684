"""The colour conversion that DEFINES cb_resize_pack_yuv420, restated in numpy float32 -- the yardstick of tests/test_yuv_ingest.py.

A YUV 4:2:0 frame (I420: Y, U, V planes; NV12: Y, interleaved UV; chroma planes of ceil(h / 2) x ceil(w / 2)) stands for the uint8 RGB
frame in which pixel (i, j) is converted from Y(i, j) and the chroma sample (i >> 1, j >> 1) -- nearest replication, what libswscale's
unscaled yuv420p -> rgb24 path does -- in fp32, every multiply and add rounded on its own in the written left-to-right order, then rounded
to nearest even and clamped to 0..255.  numpy evaluates float32 arrays operation by operation, so what stands below is that arithmetic."""
import numpy as np

f32 = np.float32
# matrix -> (limited range?, cr -> R, cb -> G, cr -> G, cb -> B)
MATRICES = {"bt601": (True, 1.596027, 0.391762, 0.812968, 2.017232),
            "bt601-full": (False, 1.402, 0.344136, 0.714136, 1.772),
            "bt709": (True, 1.792741, 0.213249, 0.532909, 2.112402),
            "bt709-full": (False, 1.5748, 0.187324, 0.468124, 1.8556)}
EXTREMES = (0, 16, 128, 235, 240, 255)


def convert(y, u, v, matrix: str) -> np.ndarray:
    """uint8 Y, U, V arrays of one shape (4:4:4) -> uint8 (3, *shape) R, G, B"""
    limited, rv, gu, gv, bu = MATRICES[matrix]
    yy = y.astype(f32)
    if limited:
        yy = f32(1.164383) * (yy - f32(16))
    cb, cr = u.astype(f32) - f32(128), v.astype(f32) - f32(128)
    r = yy + f32(rv) * cr
    g = yy - f32(gu) * cb - f32(gv) * cr
    b = yy + f32(bu) * cb
    assert r.dtype == g.dtype == b.dtype == f32
    return np.stack([np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (r, g, b)])


def chroma_shape(h: int, w: int):
    return (h + 1) // 2, (w + 1) // 2


def frame_bytes(h: int, w: int) -> int:
    ch, cw = chroma_shape(h, w)
    return h * w + 2 * ch * cw


def planes_to_rgb(y, u, v, matrix: str) -> np.ndarray:
    """Y (h, w), U, V (ch, cw) uint8 -> planar RGB uint8 (3, h, w), chroma sample (i >> 1, j >> 1) for pixel (i, j)"""
    h, w = y.shape
    assert u.shape == v.shape == chroma_shape(h, w)
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w]
    return convert(y, up(u), up(v), matrix)


def pack(y, u, v, layout: str) -> np.ndarray:
    """planes -> the frame's bytes: I420 = Y, U, V; NV12 = Y, then U and V interleaved sample by sample"""
    chroma = np.concatenate([u.ravel(), v.ravel()]) if layout == "i420" else np.stack([u, v], axis=-1).ravel()
    return np.concatenate([y.ravel(), chroma])


def unpack(frame, h: int, w: int, layout: str):
    """a frame's bytes -> (Y, U, V) planes"""
    ch, cw = chroma_shape(h, w)
    frame = np.asarray(frame)
    assert frame.shape == (frame_bytes(h, w),)
    y, c = frame[:h * w].reshape(h, w), frame[h * w:]
    if layout == "i420":
        return y, c[:ch * cw].reshape(ch, cw), c[ch * cw:].reshape(ch, cw)
    c = c.reshape(ch, cw, 2)
    return y, c[..., 0], c[..., 1]


def random_planes(h: int, w: int, seed: int):
    """seeded Y, U, V planes: half of the samples uniform over 0..255, half drawn from the range limits (EXTREMES), so that saturated
    colours -- every clamp of the conversion -- occur next to ordinary ones"""
    rng = np.random.default_rng(seed)
    ch, cw = chroma_shape(h, w)

    def plane(shape):
        uniform = rng.integers(0, 256, shape)
        limits = rng.choice(EXTREMES, shape)
        return np.where(rng.random(shape) < 0.5, uniform, limits).astype(np.uint8)
    return plane((h, w)), plane((ch, cw)), plane((ch, cw))
