"""cb_copy_ranges / ops.copy_ranges: up to eight (dst, src, bytes) ranges in one launch -- the staging of a batch into the static buffers
of a captured step.  Bit-exact against torch slicing on the host emulator build and, marked `gpu`, on the device: every length class
(0, 1, 15, 16, 17, 4095, 1 MiB + 3) at every pair of source / destination byte offsets 0..15 (the 16-byte, dword and byte paths), eight
mixed ranges in one launch, 64 guard bytes on both sides of every destination, and the argument checks."""
import ctypes as C

import pytest
import torch

from clipbert_amd import _lib, ops

GUARD = 64
SMALL = (0, 1, 15, 16, 17, 4095)
BIG = (1 << 20) + 3


def _case(hw, length, s_off, d_off, seed):
    """(dst view, src view, whole destination buffer, what it must hold afterwards)"""
    g = torch.Generator().manual_seed(seed)
    src_buf = hw(torch.randint(0, 256, (length + 32,), dtype=torch.uint8, generator=g))
    dst_buf = hw(torch.randint(0, 256, (2 * GUARD + length + 32,), dtype=torch.uint8, generator=g))
    # torch's allocations are at least 64-byte aligned, so the offsets ARE the misalignments
    assert src_buf.data_ptr() % 16 == 0 and dst_buf.data_ptr() % 16 == 0
    src = src_buf[s_off:s_off + length]
    dst = dst_buf[GUARD + d_off:GUARD + d_off + length]
    want = dst_buf.clone()
    want[GUARD + d_off:GUARD + d_off + length] = src
    return dst, src, dst_buf, want


def _check(cases):
    ops.copy_ranges([(d, s) for d, s, _b, _w in cases])
    for i, (_d, _s, buf, want) in enumerate(cases):
        assert torch.equal(buf.cpu(), want.cpu()), f"range {i}: destination or its guard bytes differ"


def test_small_lengths_at_every_offset_pair(hw):
    """0, 1, 15, 16, 17 and 4095 bytes at all 16 x 16 (source, destination) misalignments: six ranges per launch"""
    for s_off in range(16):
        for d_off in range(16):
            _check([_case(hw, n, s_off, d_off, 1000 * s_off + 10 * d_off + i) for i, n in enumerate(SMALL)])


@pytest.mark.parametrize("d_off", range(16))
def test_one_mebibyte_plus_three_at_every_offset_pair(hw, d_off):
    """the many-block length at all 16 x 16 misalignments (eight source offsets per launch)"""
    for s0 in (0, 8):
        _check([_case(hw, BIG, s0 + j, d_off, 77 * d_off + s0 + j) for j in range(8)])


def test_eight_mixed_ranges_in_one_launch(hw):
    """one range >= 1 MiB beside several < 64 bytes (and an empty one): the grid is shared out by bytes, every range still arrives"""
    spec = [(3, 1, 2), (BIG + 4096, 5, 9), (63, 0, 0), (0, 4, 4), (17, 15, 3), (40, 8, 8), (4095, 2, 6), (1, 7, 7)]
    _check([_case(hw, n, s, d, 31 * i) for i, (n, s, d) in enumerate(spec)])


def test_typed_tensors_and_more_than_eight_pairs(hw):
    """ops.copy_ranges takes any contiguous tensors of equal byte size and chunks a longer list into launches of eight"""
    g = torch.Generator().manual_seed(5)
    srcs = [hw(torch.randn(3 + 7 * i, generator=g)) for i in range(9)] + [hw(torch.randint(0, 99, (4, 5), generator=g)), hw(torch.zeros(0))]
    dsts = [hw(torch.full_like(s.cpu(), 7)) for s in srcs]
    ops.copy_ranges(list(zip(dsts, srcs)))
    for d, s in zip(dsts, srcs):
        assert torch.equal(d.cpu(), s.cpu())


def test_argument_checks(hw):
    lib = _lib.get()
    stream = ops._stream(hw(torch.zeros(1)))
    buf = hw(torch.arange(256, dtype=torch.uint8))
    before = buf.clone()

    def call(pairs, n=None):
        k = max(len(pairs), 1)
        dsts = (C.c_void_p * k)(*[d for d, _s, _b in pairs])
        srcs = (C.c_void_p * k)(*[s for _d, s, _b in pairs])
        nbytes = (C.c_int64 * k)(*[b for _d, _s, b in pairs])
        return lib.cb_copy_ranges(dsts, srcs, nbytes, len(pairs) if n is None else n, stream)

    p = buf.data_ptr()
    assert call([], 0) == 0 and lib.cb_copy_ranges(None, None, None, 0, stream) == 0                 # n == 0: a no-op, arrays not read
    assert call([(None, None, 0), (p, None, 0)]) == 0                                                # null pointers with 0 bytes only
    for bad, text in (([(p, p + 128, 1)] * 9, b"0..8 ranges"), ([(p, p + 128, -1)], b"bad range 0"), ([(p, p + 128, 4), (None, p, 4)], b"bad range 1"),
                      ([(p, None, 4)], b"bad range 0"), ([(p, p + 8, 16)], b"overlaps its own source"), ([(p + 8, p, 16)], b"overlaps its own source")):
        assert call(bad) != 0
        assert text in lib.cb_last_error(), (text, lib.cb_last_error())
    assert call([(p, p + 16, 16)]) == 0                                                              # adjacent is not overlapping
    if buf.is_cuda:
        torch.cuda.synchronize()
    want = before.clone()
    want[:16] = before[16:32]
    assert torch.equal(buf.cpu(), want.cpu())
    assert lib.cb_version() >= 12
    with pytest.raises(AssertionError):
        ops.copy_ranges([(buf[:8], buf[8:12])])                                                      # byte sizes differ
