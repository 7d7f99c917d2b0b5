"""The device reader's host side, without a GPU.

csrc/aqz_unsplit.hh holds the whole address map of the un-split kernel -- which
bytes of which chunk are which bytes of a row-major frame, ragged tiles, slabs,
the XY-swapped storage order, and every source and destination bound -- in one
text that compiles for host and device; the kernels of csrc/aqz_unsplit.hip add
only the byte movers.  tests/sanitize/unsplit_sanitize.cpp runs that text with
a serial byte mover under ASan + UBSan: frames split by the product's host
split into exactly-sized heap chunks come back bit for bit in exactly-sized
heap frames, over the geometries of tests/test_gpu_reader.py plus append chunk
1, a 2-D array (the phantom dimension), tiles taller than a slab and the XY
swap.

The rest checks the host-only entry points: the shard index parse
(aqz_shard_table_parse) against aqz_shard_table, and the reader's device-memory
estimator (aqz_reader_device_bytes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aqz
from oracle_bindings import CHANNEL, SPACE, TIME, U8, U16, U64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")
UNWRITTEN = (1 << 64) - 1


def test_unsplit_map_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "unsplit_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined", "-pthread"]
    srcs = [os.path.join(REPO, "tests", "sanitize", "unsplit_sanitize.cpp")] + [
        os.path.join(CSRC, f) for f in ("aqz_geometry.cpp", "aqz_copy.cpp", "aqz_hostsplit.cpp")]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC, *srcs, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert "clean: 44 cases" in r.stdout      # 11 geometries x 4 element sizes
    assert "runtime error" not in r.stderr


def test_shard_table_round_trip():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64):
        off = rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
        ext = rng.integers(1, 1 << 30, size=n, dtype=np.uint64)
        for i in range(0, n, 3):              # chunks never written
            off[i] = ext[i] = UNWRITTEN
        table = aqz.shard_table(off, ext)
        assert len(table) == 16 * n + 4
        got_off, got_ext, ok = aqz.shard_table_parse(table, n)
        assert ok
        assert np.array_equal(got_off, off) and np.array_equal(got_ext, ext)
        assert got_off[0] == UNWRITTEN and got_ext[0] == UNWRITTEN
        # the bytes themselves: little-endian pairs, then the CRC-32C of them
        pairs = np.frombuffer(table[:16 * n], dtype="<u8").reshape(n, 2)
        assert np.array_equal(pairs[:, 0], off) and np.array_equal(pairs[:, 1], ext)
        assert int.from_bytes(table[16 * n:], "little") == aqz.crc32c(table[:16 * n])


def test_shard_table_flipped_byte_fails_the_crc():
    off = np.arange(5, dtype=np.uint64) * 1000
    ext = np.full(5, 999, dtype=np.uint64)
    table = bytearray(aqz.shard_table(off, ext))
    for pos in (0, 37, 79, 80, 83):            # in the pairs and in the CRC itself
        bad = bytearray(table)
        bad[pos] ^= 0x10
        got_off, got_ext, ok = aqz.shard_table_parse(bytes(bad), 5)
        assert not ok, pos
        if pos >= 80:                          # the pairs are still handed back
            assert np.array_equal(got_off, off) and np.array_equal(got_ext, ext)


def test_shard_table_wrong_size_is_invalid_argument():
    table = aqz.shard_table([0, 10], [10, 20])
    for n in (1, 3):
        with pytest.raises(aqz.AqzError) as e:
            aqz.shard_table_parse(table, n)
        assert e.value.status == 1
    with pytest.raises(aqz.AqzError) as e:
        aqz.shard_table_parse(table[:-1], 2)
    assert e.value.status == 1
    assert aqz.lib().aqz_last_error()
    # null table, and outputs that may be left out
    L = aqz.lib()
    assert L.aqz_shard_table_parse(None, 36, 2, None, None, None) == 1
    buf = np.frombuffer(table, dtype=np.uint8)
    assert L.aqz_shard_table_parse(buf.ctypes.data, 36, 2, None, None, None) == 0


def _round16(n):
    return (n + 15) // 16 * 16


def test_reader_device_bytes_estimator():
    dims = [(TIME, 0, 2, 1), (CHANNEL, 3, 2, 1), (SPACE, 5, 2, 2), (SPACE, 20, 8, 1),
            (SPACE, 24, 16, 1)]
    F, n, bpc = 2 * 3 * 5, 2 * 3 * 3 * 2, 2 * 2 * 2 * 8 * 16 * 2
    words = n * 8 + (n + 1) * 8 + 2 * n * 4
    tables = F * 12 + words
    staging = aqz.compressor_max_bytes(bpc, n)
    raw = aqz.reader_device_bytes(dims, U16)
    assert raw == tables + staging
    assert aqz.reader_device_bytes(dims, U16, max_frames_bytes=4096) == tables + 4096
    for codecs in (aqz.DECODE_CODEC_LZ4, aqz.DECODE_CODEC_ZSTD,
                   aqz.DECODE_CODEC_LZ4 | aqz.DECODE_CODEC_ZSTD):
        want = raw + _round16(bpc) * n + aqz.decompressor_scratch_bytes(bpc, n, codecs)
        assert aqz.reader_device_bytes(dims, U16, codecs=codecs) == want
    # a storage order changes nothing; the element size scales the chunks
    assert aqz.reader_device_bytes(dims, U16, storage_order=[0, 2, 1, 3, 4]) == raw
    assert aqz.reader_device_bytes(dims, U64) > aqz.reader_device_bytes(dims, U8) > 0
    # a 2-D array
    assert aqz.reader_device_bytes([(SPACE, 45, 16, 1), (SPACE, 70, 32, 1)], U8) > 0


def test_reader_device_bytes_is_zero_for_invalid_descriptions():
    ok = [(TIME, 0, 2, 1), (SPACE, 64, 32, 1), (SPACE, 64, 32, 1)]
    assert aqz.reader_device_bytes(ok, U16) > 0
    assert aqz.reader_device_bytes(ok, 99) == 0                      # data type
    assert aqz.reader_device_bytes(ok, U16, codecs=4) == 0            # unknown codec bit
    assert aqz.reader_device_bytes(ok[:1], U16) == 0                  # one dimension
    assert aqz.reader_device_bytes([(TIME, 0, 2, 1), (SPACE, 64, 0, 1), (SPACE, 64, 32, 1)],
                                   U16) == 0                          # chunk size 0
    assert aqz.reader_device_bytes([(TIME, 0, 2, 1), (CHANNEL, 64, 32, 1), (SPACE, 64, 32, 1)],
                                   U16) == 0                          # y not spatial
    assert aqz.reader_device_bytes(ok, U16, storage_order=[1, 0, 2]) == 0
    assert aqz.lib().aqz_reader_device_bytes(None) == 0
    # creation refuses the same descriptions with a status, before touching a device
    h = C.c_void_p()
    d, _keep = aqz._reader_desc(ok, U16, None, 4, 0, 0)
    assert aqz.lib().aqz_reader_create(C.byref(d), C.byref(h)) == 1
    assert not h.value
