"""Region reads on the host, without a GPU.

csrc/aqz_unsplit.hh's region part -- the region in storage coordinates, the item
walk over the tiles and slabs that meet it, region_rect's clip and every bound --
runs in tests/sanitize/region_sanitize.cpp with a serial byte mover under ASan +
UBSan: chunks outside the region's chunk set are not allocated at all, and the
destination is exactly as large as the crop with its strides.

aqz_dims_region_chunks is checked against the oracle's write path: frames that
are zero outside the region and nonzero inside it set has_data for exactly the
chunks of the set."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aqz
import oracle_bindings as ob
from oracle_bindings import NP_DTYPES, U8, U16, U64, OracleDims
from region_helpers import (GEOMETRIES, PERMUTED, XY_ORDER, XY_SHAPES, frame_ranges,
                            regions_of, xy_dims)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")


def test_region_map_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "region_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-pthread"]
    srcs = [os.path.join(REPO, "tests", "sanitize", "region_sanitize.cpp")] + [
        os.path.join(CSRC, f) for f in ("aqz_geometry.cpp", "aqz_copy.cpp", "aqz_hostsplit.cpp",
                                        "aqz_region.cpp")]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC, *srcs, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    # (geometry, element size, region): the 11 geometries of unsplit_sanitize.cpp and a
    # taller one x 4 sizes x 8 regions; tiles above 64 rows add 3 slab regions
    # (tall-tiles, xy-tall) or 4 (taller-tiles: rows 60-70 of tile row 1 exist there)
    assert "clean: 424 cases" in r.stdout
    assert "runtime error" not in r.stderr


CASES = [(name, dims, None) for name, dims in GEOMETRIES.items()] + \
        [("5d-permuted",) + PERMUTED] + \
        [("xy-%dx%d" % s[:2], xy_dims(s), XY_ORDER) for s in XY_SHAPES]


@pytest.mark.parametrize("name,dims,order", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("dtype", [U8, U16])
def test_region_chunks_are_the_chunks_the_oracle_writes(name, dims, order, dtype):
    """Frames that are nonzero exactly inside the region, written by the oracle's
    write_frame_to_chunks (storage dims; the storage frame id from
    transpose_frame_id, pinned to the reference in tests/test_host_cpu.py; an
    XY-swapped frame transposed as transpose_frame does): has_data is set for
    exactly the chunks of aqz_dims_region_chunks."""
    d = aqz.Dims(dims, dtype, storage_order=order)
    storage = [dims[i] for i in order] if order else dims
    xy = order is not None and order[-2:] != [len(dims) - 2, len(dims) - 1]
    od = OracleDims(storage, dtype)
    F = od.frames_per_chunk_layer()
    assert F == d.frames_per_chunk_layer()
    n = od.number_of_chunks_in_memory()
    H, W = dims[-2][1], dims[-1][1]
    regions = regions_of(dims, "x" if xy else "y")
    assert len(regions) >= 8
    for rname, (x0, y0, w, h) in regions.items():
        frame = np.zeros((H, W), dtype=NP_DTYPES[dtype])
        frame[y0:y0 + h, x0:x0 + w] = 1
        sframe = np.ascontiguousarray(frame.T) if xy else frame
        for first, count in frame_ranges(F):
            buf, has = od.new_layer()
            for f in range(first, first + count):
                od.write_frame_to_chunks(d.transpose_frame_id(f), sframe, buf, has)
            want = np.flatnonzero(has).astype(np.uint32)
            got = d.region_chunks(first, count, (x0, y0, w, h))
            assert got.dtype == np.uint32 and np.array_equal(got, want), \
                (name, rname, first, count, got, want)
            assert 0 < len(got) <= n and (np.diff(got.astype(np.int64)) > 0).all()


def _call(d, first, count, region, chunks, cap, n):
    reg = None if region is None else C.byref(aqz.RegionC(*region))
    return aqz.lib().aqz_dims_region_chunks(d, first, count, reg, chunks, cap, n)


def test_region_chunks_refusals():
    dims = GEOMETRIES["ragged"]                      # 45 rows of 70 pixels, 3 frames a layer
    d = aqz.Dims(dims, U16)
    L = aqz.lib()
    out = (C.c_uint32 * 16)()
    n = C.c_uint32(77)

    def refused(h, first, count, region, count_out=C.byref(n)):
        status = _call(h, first, count, region, out, 16, count_out)
        assert status == 1, (first, count, region)
        assert L.aqz_last_error()

    refused(d.h, 0, 1, None)                         # NULL region
    refused(None, 0, 1, (0, 0, 1, 1))                # NULL dims
    refused(d.h, 0, 1, (0, 0, 1, 1), count_out=None)  # NULL n
    refused(d.h, 0, 1, (0, 0, 0, 1))                 # zero width
    refused(d.h, 0, 1, (0, 0, 1, 0))                 # zero height
    refused(d.h, 0, 1, (0xffffffff, 0, 2, 1))        # x0 + width wraps in 32 bits
    refused(d.h, 0, 1, (0, 0xffffffff, 1, 2))        # y0 + height wraps
    refused(d.h, 0, 1, (69, 0, 2, 1))                # one pixel past the row
    refused(d.h, 0, 1, (0, 44, 1, 2))                # one row past the frame
    refused(d.h, 0, 0, (0, 0, 1, 1))                 # count == 0
    refused(d.h, 3, 1, (0, 0, 1, 1))                 # outside frames_per_chunk_layer
    refused(d.h, 2, 2, (0, 0, 1, 1))
    refused(d.h, 0xffffffff, 2, (0, 0, 1, 1))        # first + count wraps
    assert n.value == 0                              # no count from a refused call
    # the edges themselves are accepted
    assert _call(d.h, 2, 1, (68, 43, 2, 2), out, 16, C.byref(n)) == 0 and n.value == 1
    # cap too small: the status aqz_reader_status gives a short array, and the count needed
    whole = (0, 0, 70, 45)
    assert _call(d.h, 0, 3, whole, out, 16, C.byref(n)) == 0
    need = n.value
    assert need == d.number_of_chunks_in_memory() == 9
    n.value = 0
    assert _call(d.h, 0, 3, whole, out, need - 1, C.byref(n)) == 2
    assert n.value == need and L.aqz_last_error()
    n.value = 0
    assert _call(d.h, 0, 3, whole, None, 0, C.byref(n)) == 0 and n.value == need  # count only
    with pytest.raises(aqz.AqzError) as e:
        d.region_chunks(0, 1, (0, 0, 71, 1))
    assert e.value.status == 1
    assert aqz.DECODE_NOT_LOADED == 5
