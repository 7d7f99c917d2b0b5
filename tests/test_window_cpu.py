"""The byte hull of a window inside its chunks, without a GPU.

aqz_dims_region_chunk_ranges gives, for every chunk of aqz_dims_region_chunks, the
smallest interval [lo, hi) of chunk bytes that holds every byte a crop reads.  It is
checked against brute force: u32 frames whose pixel value is its own linear index in
the layer (plus one, so that chunk padding, zero, is no pixel) are split into chunks
by the oracle's write path; the pixels of a crop are then found again in every chunk,
and the first and the last of their byte positions must be lo and hi - 1."""
import ctypes as C

import numpy as np
import pytest

import aqz
from oracle_bindings import U16, U32, OracleDims
from region_helpers import (GEOMETRIES, PERMUTED, XY_ORDER, XY_SHAPES, frame_ranges,
                            regions_of, xy_dims)

CASES = [(name, dims, None) for name, dims in GEOMETRIES.items()] + \
        [("5d-permuted",) + PERMUTED] + \
        [("xy-%dx%d" % s[:2], xy_dims(s), XY_ORDER) for s in XY_SHAPES]


@pytest.mark.parametrize("name,dims,order", CASES, ids=[c[0] for c in CASES])
def test_hull_is_the_first_and_last_byte_of_the_crop_in_every_chunk(name, dims, order):
    d = aqz.Dims(dims, U32, storage_order=order)
    storage = [dims[i] for i in order] if order else dims
    xy = order is not None and order[-2:] != [len(dims) - 2, len(dims) - 1]
    od = OracleDims(storage, U32)
    F = od.frames_per_chunk_layer()
    n = od.number_of_chunks_in_memory()
    bpc = od.bytes_per_chunk()
    assert F == d.frames_per_chunk_layer() and F * dims[-2][1] * dims[-1][1] < 1 << 32
    H, W = dims[-2][1], dims[-1][1]
    frames = (np.arange(F * H * W, dtype=np.uint32) + 1).reshape(F, H, W)
    buf, has = od.new_layer()
    for f in range(F):
        sframe = np.ascontiguousarray(frames[f].T) if xy else frames[f]
        od.write_frame_to_chunks(d.transpose_frame_id(f), sframe, buf, has)
    chunks = buf.view(np.uint32).reshape(n, bpc // 4)
    regions = regions_of(dims, "x" if xy else "y")
    assert len(regions) >= 8
    for rname, (x0, y0, w, h) in regions.items():
        for first, count in frame_ranges(F):
            crop = frames[first:first + count, y0:y0 + h, x0:x0 + w].ravel()
            want_chunks, want = [], []
            for c in range(n):
                at = np.flatnonzero(np.isin(chunks[c], crop))
                if len(at):
                    want_chunks.append(c)
                    want.append((int(at[0]) * 4, int(at[-1]) * 4 + 4))
            got_chunks, got = d.region_chunk_ranges(first, count, (x0, y0, w, h))
            what = (name, rname, first, count)
            assert got_chunks.dtype == np.uint32 and got.dtype == np.uint64
            assert np.array_equal(got_chunks, d.region_chunks(first, count, (x0, y0, w, h))), what
            assert got_chunks.tolist() == want_chunks, what
            assert [tuple(r) for r in got.tolist()] == want, what
            assert (got[:, 0] < got[:, 1]).all() and (got[:, 1] <= bpc).all(), what


def _call(d, first, count, region, chunks, ranges, cap, n):
    reg = None if region is None else C.byref(aqz.RegionC(*region))
    return aqz.lib().aqz_dims_region_chunk_ranges(d, first, count, reg, chunks, ranges, cap, n)


def test_chunk_ranges_refusals_and_overflow():
    """The argument checks, the overflow rule and the error texts of
    aqz_dims_region_chunks (tests/test_region_cpu.py)."""
    dims = GEOMETRIES["ragged"]                      # 45 rows of 70 pixels, 3 frames a layer
    d = aqz.Dims(dims, U16)
    L = aqz.lib()
    chunks = (C.c_uint32 * 16)()
    ranges = (aqz.ByteRangeC * 16)()
    n = C.c_uint32(77)

    def refused(h, first, count, region, count_out=C.byref(n)):
        assert _call(h, first, count, region, chunks, ranges, 16, count_out) == 1, \
            (first, count, region)
        text = L.aqz_last_error()
        assert text
        return text.decode()

    def same_text(first, count, region):
        got = refused(d.h, first, count, region)
        reg = None if region is None else C.byref(aqz.RegionC(*region))
        assert L.aqz_dims_region_chunks(d.h, first, count, reg, chunks, 16, C.byref(n)) == 1
        assert L.aqz_last_error().decode() == got

    same_text(0, 1, None)                            # NULL region
    refused(None, 0, 1, (0, 0, 1, 1))                # NULL dims
    refused(d.h, 0, 1, (0, 0, 1, 1), count_out=None)  # NULL n
    same_text(0, 1, (0, 0, 0, 1))                    # zero width
    same_text(0, 1, (0, 0, 1, 0))                    # zero height
    same_text(0, 1, (0xffffffff, 0, 2, 1))           # x0 + width wraps in 32 bits
    same_text(0, 1, (0, 0xffffffff, 1, 2))           # y0 + height wraps
    same_text(0, 1, (69, 0, 2, 1))                   # one pixel past the row
    same_text(0, 1, (0, 44, 1, 2))                   # one row past the frame
    same_text(0, 0, (0, 0, 1, 1))                    # count == 0
    same_text(3, 1, (0, 0, 1, 1))                    # outside frames_per_chunk_layer
    same_text(2, 2, (0, 0, 1, 1))
    same_text(0xffffffff, 2, (0, 0, 1, 1))           # first + count wraps
    assert n.value == 0                              # no count from a refused call
    # the edges themselves are accepted: the last two pixels of the last two rows
    assert _call(d.h, 2, 1, (68, 43, 2, 2), chunks, ranges, 16, C.byref(n)) == 0
    assert n.value == 1 and chunks[0] == 8 + 0 * 9
    # cap too small: AQZ_STATUS_OVERFLOW, and the count needed
    whole = (0, 0, 70, 45)
    assert _call(d.h, 0, 3, whole, chunks, ranges, 16, C.byref(n)) == 0
    need = n.value
    assert need == d.number_of_chunks_in_memory() == 9
    for args in ((chunks, ranges), (chunks, None), (None, ranges)):
        n.value = 0
        assert _call(d.h, 0, 3, whole, *args, need - 1, C.byref(n)) == 2
        assert n.value == need and L.aqz_last_error()
    n.value = 0
    assert _call(d.h, 0, 3, whole, None, None, 0, C.byref(n)) == 0 and n.value == need
    # one array alone is filled
    ranges[0].hi = 0
    assert _call(d.h, 0, 3, whole, None, ranges, 16, C.byref(n)) == 0 and ranges[0].hi > 0
    with pytest.raises(aqz.AqzError) as e:
        d.region_chunk_ranges(0, 1, (0, 0, 71, 1))
    assert e.value.status == 1
    assert C.sizeof(aqz.ByteRangeC) == 16
