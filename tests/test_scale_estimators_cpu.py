"""The memory estimators at the counts and sizes where a 32-bit product would wrap
(aqz_compressor_max_bytes, aqz_compressor_scratch_bytes,
aqz_decompressor_scratch_bytes_for, aqz_reader_device_bytes), against a restatement
in Python integers, which cannot wrap.  No GPU: the estimators are host code.

The cases: the largest chunk blosc1 allows (0x7fffffef bytes) three times, five
1 GiB chunks (frames past 4 GiB), and 65535 / 70000 chunks of 64 bytes (chunk
counts at and past 2^16).  Most expected values lie above 2^32 -- the test says
which -- so a library that dropped to 32 bits in any of these products fails."""
import pytest

import aqz
from oracle_bindings import SPACE, TIME, U8
from zstdpar_helpers import parallel_scratch_bytes

CASES = [(0x7fffffef, 3), (1 << 30, 5), (64, 65535), (64, 70000)]

LZ4, BLOSC_ZSTD, ZSTD = aqz.CODEC_BLOSC_LZ4, aqz.CODEC_BLOSC_ZSTD, aqz.CODEC_ZSTD
Z, P = aqz.DECODE_CODEC_ZSTD, aqz.DECODE_ZSTD_PARALLEL

# csrc/aqz_zstd.hh, aqz_codec.hh, aqz_hostzstd.hh
ZBLOCK = 8 * 1024            # zstd::kBlock: bytes per zstd block of the device encoder
ZSUB = 4096                  # kZSub: bytes per parse unit
ZSUB_SEQ = 1024              # kZSubSeq: sequences a parse unit holds
LZ4_STREAM = 4096            # kLz4StreamMax
BLOSC_ZSTD_BLOCK = 256 * 1024  # kZstdBlock


def _fse_table(log):
    """sizeof(zstd::FseTable<log>): uint16 st[1 << log], uint32 dnb[53], int32 dfs[53],
    uint32 al."""
    return 2 * (1 << log) + 4 * 53 + 4 * 53 + 4


SEG_TABLE = 16 + 2 * 256 + 256 + 160          # sizeof(ZstdSegTable)
SEQ_SEG = 16 + 256 + 3 * _fse_table(9)        # sizeof(ZstdSeqSeg)
SEQ_TABLES = 3 * _fse_table(6)                # sizeof(zstd::SeqTables)


def r16(v):
    return (v + 15) // 16 * 16


def max_bytes(cb, n):
    """Compressor::max_bytes (csrc/aqz_engine.hh)."""
    return n * (cb + 32 + 3 * (cb // ZBLOCK + 1))


def blosc_geom(nbytes, ts):
    """(streams per chunk, slot bytes) of make_blosc_geom (csrc/aqz_codec.hip)."""
    bs = min(LZ4_STREAM * ts, nbytes)
    bs -= bs % ts
    if bs == 0:
        bs = nbytes
    nfull, left = nbytes // bs, nbytes % bs
    ns_full = ts if ts <= 16 and bs // ts >= 128 else 1
    return nfull * ns_full + (1 if left else 0), max(bs // ns_full, left)


def huf_group_log2(shuffle, ts, seg, clevel):
    """zstd_huf_group_log2 (csrc/aqz_codec.hh)."""
    if shuffle == 0:
        return 5
    lg = 3
    if shuffle == 2 and clevel >= 7:
        plane = seg // (8 * ts)
        while lg > 0 and (ZBLOCK << lg) > plane:
            lg -= 1
    return lg


def far_slices(codec, clevel, shuffle):
    """zstd_far_slices (csrc/aqz_engine.cpp)."""
    if codec == ZSTD:
        zl = 3 if clevel == 0 else clevel
        return 8 if zl >= 7 else 4 if zl >= 3 else 0
    return 1 if codec == BLOSC_ZSTD and shuffle == 2 and clevel >= 2 else 0


def compressor_scratch(codec, clevel, shuffle, cb, ts, n):
    """Compressor::scratch_bytes (csrc/aqz_engine.cpp)."""
    store_only = codec != ZSTD and clevel == 0
    b = n * 4 + n + n * 8
    if codec == LZ4:
        spc, slot = blosc_geom(cb, ts)
        ns = n * spc
        return b + (1 if store_only else ns * slot) + ns * 8
    seg, nseg1 = cb, 1
    if codec == BLOSC_ZSTD:
        bs = min(BLOSC_ZSTD_BLOCK, cb)
        bs -= bs % ts
        seg = bs or cb
        nseg1 = -(-cb // seg)
    nseg, bps = n * nseg1, -(-seg // ZBLOCK)
    gl = huf_group_log2(shuffle if codec == BLOSC_ZSTD else 0, ts, seg, clevel)
    nblk, ngrp = nseg * bps, nseg * ((bps + (1 << gl) - 1) >> gl)
    b += nseg * 4
    if codec == BLOSC_ZSTD and not store_only and (shuffle == 2 or (shuffle == 1 and ts > 1)):
        b += n * cb
    if store_only:
        return b
    if far_slices(codec, clevel, shuffle):
        b += nseg * seg * 4
    nu = nblk * (ZBLOCK // ZSUB)
    b += nu * ZSUB + nu * ZSUB_SEQ * 8 + 4 * nu * 4
    b += nblk * (1 + 4 + 4 + 4 + 256 * 4 + 1 + 4 + 4 + ZBLOCK)
    b += nseg * (192 * 4 + SEQ_SEG + 4 + 1 + 4)
    b += ngrp * (SEG_TABLE + 4) + SEQ_TABLES
    return b


def decoder_scratch(cb, n, codecs):
    """include/aqz_gpu.h, aqz_decompressor_scratch_bytes_for."""
    b = r16(cb) * n
    if codecs & Z:
        b += n * min(8, -(-cb // 32768)) * r16(min(cb, 128 * 1024))
    if codecs & P:
        b += parallel_scratch_bytes(cb, n)
    return b


@pytest.mark.parametrize("cb,n", CASES)
def test_compressor_max_bytes(cb, n):
    want = max_bytes(cb, n)
    assert aqz.compressor_max_bytes(cb, n) == want
    assert want >= n * (cb + 16)                      # holds n memcpyed blosc frames
    if cb >= 1 << 30:
        assert want > 1 << 32


SETTINGS = [(LZ4, 5, 0, 1), (LZ4, 5, 1, 2), (LZ4, 0, 2, 2), (BLOSC_ZSTD, 0, 1, 2),
            (BLOSC_ZSTD, 3, 1, 2), (BLOSC_ZSTD, 5, 2, 2), (BLOSC_ZSTD, 9, 2, 2),
            (ZSTD, 1, 0, 1), (ZSTD, 3, 0, 2), (ZSTD, 9, 0, 2)]


@pytest.mark.parametrize("cb,n", CASES)
def test_compressor_scratch_bytes(cb, n):
    above = 0
    for codec, clevel, shuffle, ts in SETTINGS:
        if cb % ts:
            cb_ = cb - cb % ts
        else:
            cb_ = cb
        want = compressor_scratch(codec, clevel, shuffle, cb_, ts, n)
        got = aqz.compressor_scratch_bytes((codec, clevel, shuffle), cb_, ts, n)
        assert got == want, (codec, clevel, shuffle, ts, got, want)
        above += want > 1 << 32
    # the scratch of the big chunks passes 2^32 for every setting that compresses
    if cb >= 1 << 30:
        assert above >= 8
    # invalid settings and sizes are 0, not a wrapped number
    assert aqz.compressor_scratch_bytes((LZ4, 5, 1), 0x7ffffff0, 1, n) == 0
    assert aqz.compressor_scratch_bytes((LZ4, 5, 1), (1 << 32) + 64, 1, n) == 0
    assert aqz.compressor_scratch_bytes((ZSTD, 3, 1), cb, 1, n) == 0


def test_plain_zstd_scratch_of_five_1gib_chunks():
    """Plain zstd level 1 on five chunks of 1 GiB + 48 bytes, the largest case of the
    4 GiB test (test_gpu_scale_edges.py): 20.7 GiB of compressor scratch and 20.0 GiB
    of buffers (source, frames, decoded copy, the serial decoder's scratch) stay under
    48 GiB, so the case is part of that test.  The block-parallel decoder's scratch
    alone would be 30.3 GiB: that decoder is left out of it."""
    nb, n = (1 << 30) + 48, 5
    scratch = aqz.compressor_scratch_bytes((ZSTD, 1, 0), nb, 1, n)
    assert scratch == compressor_scratch(ZSTD, 1, 0, nb, 1, n)
    buffers = n * nb + aqz.compressor_max_bytes(nb, n) + n * nb + \
        aqz.decompressor_scratch_bytes(nb, n, Z)
    assert 40 << 30 < scratch + buffers < 41 << 30
    assert 20 << 30 < scratch < 21 << 30
    assert aqz.decompressor_scratch_bytes(nb, n, Z | P) > 30 << 30


@pytest.mark.parametrize("cb,n", CASES)
def test_decompressor_scratch_bytes(cb, n):
    assert aqz.decompressor_scratch_bytes(cb, n) == r16(cb) * n
    for codecs in (aqz.DECODE_CODEC_LZ4 | Z, Z, Z | P):
        want = decoder_scratch(cb, n, codecs)
        assert aqz.decompressor_scratch_bytes(cb, n, codecs) == want, (codecs, want)
        if cb >= 1 << 30:
            assert want > 1 << 32
    assert aqz.decompressor_scratch_bytes(0x7ffffff0, n, Z) == 0
    assert aqz.decompressor_scratch_bytes((1 << 32) + 64, n, Z) == 0


# U8 arrays whose level-0 chunk layer has exactly (chunk bytes, chunks) of CASES:
# 0x7fffffef = 3 * 36031 * 19867 (36031 = 137 * 263)
READER_DIMS = {
    (0x7fffffef, 3): ([(TIME, 0, 3, 1), (SPACE, 36031, 36031, 1), (SPACE, 3 * 19867, 19867, 1)], 3),
    (1 << 30, 5): ([(TIME, 0, 1, 1), (SPACE, 32768, 32768, 1), (SPACE, 5 * 32768, 32768, 1)], 1),
    (64, 65535): ([(TIME, 0, 1, 1), (SPACE, 8 * 255, 8, 1), (SPACE, 8 * 257, 8, 1)], 1),
    (64, 70000): ([(TIME, 0, 1, 1), (SPACE, 8 * 250, 8, 1), (SPACE, 8 * 280, 8, 1)], 1),
}


@pytest.mark.parametrize("cb,n", CASES)
def test_reader_device_bytes(cb, n):
    dims, F = READER_DIMS[(cb, n)]
    tables = F * 12 + n * 8 + (n + 1) * 8 + 2 * n * 4
    raw = tables + max_bytes(cb, n)
    assert aqz.reader_device_bytes(dims, U8) == raw
    assert aqz.reader_device_bytes(dims, U8, max_frames_bytes=1 << 33) == tables + (1 << 33)
    for codecs in (aqz.DECODE_CODEC_LZ4, Z, Z | P):
        want = raw + r16(cb) * n + decoder_scratch(cb, n, codecs)
        assert aqz.reader_device_bytes(dims, U8, codecs=codecs) == want, codecs
        if cb >= 1 << 30:
            assert want > 3 << 32
    # one byte per chunk more than blosc1 allows
    if cb == 0x7fffffef:
        over = [dims[0], (SPACE, 36031, 36031, 1), (SPACE, 3 * 19868, 19868, 1)]
        assert aqz.reader_device_bytes(over, U8) == 0
