"""cb_resize_pack_u8_src / cb_resize_pack_yuv420_src (the raw-frame ingest from a buffer NAMED IN DEVICE MEMORY: cb_frame_source) and
cb_resize_table_check (the direct entry points' row rules as a host-only function).

The _src entry points are defined through the direct ones: for the same bytes, table and parameters the output is bit-equal, so every
comparison below is torch.equal on the bytes -- no tolerance.  Geometry: three frames of 5 x 7, 8 x 6 and 1 x 9 in one buffer at S = 8,
pad 3, extra_w 2 (odd sizes: the chroma planes round up; the 1 x 9 frame resizes to a height of 0 by get_resize_size, which no table may
carry, so its row says 1 x 8).  On the emulator a read is a real host read: the bounds tests put a canary of 255s behind the bytes the
descriptor admits, and 255 never normalises to the padding pixel."""
import pytest
import torch

import resize_restatement as R
from clipbert_amd import _lib, data, ops

MEAN, STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
S, PAD, EXTRA_W = 8, 3, 2
SIZES = [(5, 7), (8, 6), (1, 9)]
SOURCES = ("hwc", "planar", "i420", "nv12")
MATRICES = ("bt601", "bt709-full")


def _frame_bytes(kind, h, w):
    return 3 * h * w if kind in ("hwc", "planar") else data.yuv420_frame_bytes(h, w)


def _batch(kind, sizes=SIZES, seed=0):
    """(flat uint8 bytes, (n, 5) table) of random frames lying back to back"""
    rows, off = [], 0
    for h, w in sizes:
        nh, nw = data.resize_size(h, w, S)
        rows.append([off, h, w, max(nh, 1), max(nw, 1)])
        off += _frame_bytes(kind, h, w)
    flat = torch.randint(0, 256, (off,), dtype=torch.uint8, generator=torch.Generator().manual_seed(17 * seed + len(kind)))
    return flat, torch.tensor(rows, dtype=torch.int64)


def _call(kind, flat, table, dtype, matrix="bt601", host_table=None, source=None):
    n = table.shape[0]
    if kind in ("hwc", "planar"):
        return ops.resize_pack_u8(flat, table, n, S, dtype, MEAN, STD, hwc=kind == "hwc", pad=PAD, extra_w=EXTRA_W, host_table=host_table, source=source)
    return ops.resize_pack_yuv420(flat, table, n, S, dtype, MEAN, STD, layout=kind, matrix=matrix, pad=PAD, extra_w=EXTRA_W, host_table=host_table,
                                  source=source)


def _desc(hw, flat, nbytes=None):
    """an int64 (2,) cb_frame_source on the backend's device naming the first ``nbytes`` bytes of ``flat``"""
    return hw(torch.tensor([flat.data_ptr(), flat.numel() if nbytes is None else nbytes], dtype=torch.int64))


def _bytes(t):
    return t.cpu().contiguous().view(torch.uint8)


def _pad_only(dtype):
    """ImagePad's zero pixel, normalised, inside S x S; zeros in the halo"""
    return R.packed_reference(torch.zeros(1, 3, S, S), [(0, 0)], MEAN, STD, PAD, EXTRA_W)[0][0].to(dtype)


# ---- 1. bit-equality with the direct entry points -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", SOURCES)
def test_source_launch_equals_direct_launch(hw, kind, dtype):
    flat, table = _batch(kind)
    flat_d, table_d = hw(flat), hw(table)
    for matrix in (MATRICES if kind in ("i420", "nv12") else ("bt601",)):
        want = _call(kind, flat_d, table_d, dtype, matrix, host_table=table)
        for desc in (_desc(hw, flat_d), _desc(hw, flat_d).view(torch.uint8)):                   # int64 (2,) and uint8 (16,)
            got = _call(kind, None, table_d, dtype, matrix, source=desc)
            assert got.shape == want.shape == (3, S + 2 * PAD, S + 2 * PAD + EXTRA_W, 4) and got.dtype == dtype
            assert torch.equal(_bytes(got), _bytes(want)), (kind, matrix)
        assert not torch.equal(want[0].cpu(), _pad_only(dtype))                                  # (the frames are not padding)


# ---- 2. bounds ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", SOURCES)
def test_empty_descriptor_is_all_padding_and_reads_nothing(hw, kind, dtype):
    _, table = _batch(kind)
    pad_only = _pad_only(dtype)
    canary = hw(torch.full((4096,), 255, dtype=torch.uint8))                                     # what base points at must not be read
    for desc in (hw(torch.zeros(2, dtype=torch.int64)), _desc(hw, canary, 0)):
        got = _call(kind, None, hw(table), dtype, source=desc).cpu()
        for f in range(3):
            assert torch.equal(got[f], pad_only), (kind, f)


@pytest.mark.parametrize("kind", SOURCES)
def test_descriptor_ending_inside_the_last_frame_pads_that_frame_only(hw, kind):
    flat, table = _batch(kind)
    true = flat.numel()
    cut = true - 5                                                                               # inside the 1 x 9 frame
    assert table[2, 0] < cut < true
    if hw.name == "emul":
        # the bytes past `cut` -- the frame's tail and everything behind the buffer -- are a canary: an out-of-range read would be a real read
        whole = torch.cat([flat[:cut], torch.full((true - cut + 4096,), 255, dtype=torch.uint8)])
        flat_d = whole[:true]
    else:
        flat_d = hw(flat)                                                                        # its true size, nothing behind it
    table_d = hw(table)
    got = _call(kind, None, table_d, torch.float32, source=_desc(hw, flat_d, cut)).cpu()
    direct = _call(kind, flat_d[:cut], table_d, torch.float32).cpu()                             # table_host=None, the same flat_bytes
    full = _call(kind, flat_d, table_d, torch.float32, host_table=table).cpu()
    assert torch.equal(got, direct)
    assert torch.equal(got[2], _pad_only(torch.float32))
    assert torch.equal(got[:2], full[:2]) and not torch.equal(full[2], got[2])
    # no output pixel of the padded frame carries the canary: (255 - mean) * (1 / std) is positive in every channel, the padding negative
    assert float(got[2].max()) <= 0.0


# ---- 3. resize_table_check ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hwc", "i420"])
def test_table_check_accepts_a_collated_table_and_rejects_what_the_direct_launch_rejects(hw, kind):
    pixfmt = "rgb" if kind == "hwc" else kind
    g = torch.Generator().manual_seed(5)
    if kind == "hwc":
        rf = data.collate_raw_frames([torch.randint(0, 256, (2, 5 + v, 7, 3), dtype=torch.uint8, generator=g) for v in range(2)], S)
    else:
        rf = data.collate_yuv_frames([(torch.randint(0, 256, (2, data.yuv420_frame_bytes(5 + v, 7)), dtype=torch.uint8, generator=g), 5 + v, 7)
                                      for v in range(2)], S, layout=kind)
    _, host = rf.packed_table()
    n, nbytes = rf.n_frames, rf.flat.numel()
    ops.resize_table_check(host, n, nbytes, S, pixfmt)
    off, h, w, nh, nw = (int(x) for x in host[1])
    bad_rows = [[off, 0, w, nh, nw],                                                             # h = 0
                [off, h, w, nh, S + 1],                                                          # new_w = S + 1
                [nbytes - _frame_bytes(kind, h, w) + 1, h, w, nh, nw],                           # the frame leaves the buffer
                [-1, h, w, nh, nw]]                                                              # a negative offset
    flat_d = hw(rf.flat)
    for row in bad_rows:
        bad = host.clone()
        bad[1] = torch.tensor(row)
        with pytest.raises(RuntimeError) as direct:
            _call(kind, flat_d, hw(bad), torch.float32, host_table=bad)
        with pytest.raises(RuntimeError) as check:
            ops.resize_table_check(bad, n, nbytes, S, pixfmt)
        assert str(check.value) == str(direct.value) and "frame 1" in str(check.value), (row, str(check.value), str(direct.value))
    for kw, message in ((dict(n=0), "bad N"), (dict(pixfmt=3), "bad pixfmt")):
        args = dict(dict(n=n, pixfmt=_lib.PIXFMTS[pixfmt]), **kw)
        assert _lib.get().cb_resize_table_check(host.data_ptr(), args["n"], nbytes, S, args["pixfmt"]) != 0
        assert message in _lib.get().cb_last_error().decode(), kw


def test_source_entry_points_refuse_bad_arguments_and_launch_nothing(hw):
    import ctypes as C
    flat, table = _batch("hwc")
    flat_d, table_d = hw(flat), hw(table)
    desc = _desc(hw, flat_d)
    hp, wp = S + 2 * PAD, S + 2 * PAD + EXTRA_W
    dst = hw(torch.full((3, hp, wp, 4), 7.0))
    mean, std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)
    lib = _lib.get()

    def u8(src=ops._ptr(desc), n=3, s=S, pad=PAD, dtype=_lib.CB_F32, table=ops._ptr(table_d)):
        return lib.cb_resize_pack_u8_src(dtype, src, table, n, 1, mean, std, ops._ptr(dst), s, hp, wp, pad, ops._stream(dst))

    for kw, message in ((dict(src=None), "null operand"), (dict(table=None), "null operand"), (dict(src=ops._ptr(desc) + 8), "16-byte aligned"),
                        (dict(n=0), "bad N"), (dict(n=65536), "bad N"), (dict(s=0), "bad N"), (dict(pad=-1), "bad N"), (dict(s=S + 1), "does not hold"),
                        (dict(dtype=2), "bad dtype")):
        assert u8(**kw) != 0 and message in lib.cb_last_error().decode(), (kw, lib.cb_last_error().decode())
    yuv = lambda layout=0, matrix=0: lib.cb_resize_pack_yuv420_src(_lib.CB_F32, ops._ptr(desc), ops._ptr(table_d), 3, layout, matrix, mean, std,    # noqa: E731
                                                                   ops._ptr(dst), S, hp, wp, PAD, ops._stream(dst))
    for kw, message in ((dict(layout=2), "bad layout"), (dict(matrix=4), "bad matrix")):
        assert yuv(**kw) != 0 and message in lib.cb_last_error().decode(), kw
    assert torch.count_nonzero(dst.cpu() != 7.0) == 0
    assert u8() == 0 and torch.count_nonzero(dst.cpu() == 7.0) == 0


# ---- 4. capture one launch, then swap the source -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hwc", "nv12"])
def test_captured_launch_follows_the_descriptor(kind):
    dev = torch.device("cuda", 0)
    flat_a, table_a = _batch(kind, seed=1)
    flat_b, table_b = _batch(kind, sizes=[(9, 4), (3, 3), (6, 11)], seed=2)                      # other native sizes, another byte count
    assert flat_a.numel() != flat_b.numel()
    flat_a, flat_b = flat_a.to(dev), flat_b.to(dev)
    table = table_a.to(dev)                                                                      # the ONE table the graph reads
    source = data.FrameSource(dev)
    source.point_at(flat_a)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _call(kind, None, table, torch.bfloat16, source=source.desc)
    graph.replay()
    assert torch.equal(out, _call(kind, flat_a, table_a.to(dev), torch.bfloat16, host_table=table_a))
    table.copy_(table_b.to(dev))                                                                 # rewritten in place
    source.point_at(flat_b)
    graph.replay()
    want = _call(kind, flat_b, table_b.to(dev), torch.bfloat16, host_table=table_b)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert source.flat is flat_b                                                                 # the owner keeps what the descriptor names


# ---- 5. version and symbols ------------------------------------------------------------------------------------------------------------
def test_version_and_symbols(hw):
    lib = _lib.get()
    assert lib.cb_version() >= 17
    new = {"cb_resize_pack_u8_src", "cb_resize_pack_yuv420_src", "cb_resize_table_check"}
    assert new <= set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, s) for s in new)
