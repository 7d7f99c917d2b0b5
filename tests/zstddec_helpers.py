"""Helpers of the device zstd decoder's tests (test_zstddec_cpu.py,
test_gpu_zstddec.py, golden/make_zstd_frames.py): a header-level inspector of a
zstd frame (a restatement of RFC 8878's layout), a small hand-assembler of
frames libzstd will not emit on request, the named mutations with the status
each must get, the golden fixture's loader, and libzstd with explicit
parameters.  The seeded byte mutations and the corpus writer are
decoder_helpers'.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

from codec_helpers import header, libzstd, zstd_compress, zstd_decode
from decoder_helpers import (BAD_HEADER, CORRUPT, OK, SKIPPED, UNSUPPORTED,  # noqa: F401
                             byte_mutations, sha256, write_corpus)
from decoder_helpers import streams as blosc_streams

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zstd_frames.npz")
MAGIC = 0xFD2FB528
BLOCK_MAX = 128 * 1024
LIT_TYPES = ("raw", "rle", "compressed", "treeless")
MODES = ("predefined", "rle", "fse", "repeat")


# ---- libzstd with explicit parameters ----------------------------------------
def zstd_compress2(data: bytes, level: int, window_log: int = 0, checksum: bool = False) -> bytes:
    """ZSTD_compress2 with parameters 100 (level), 101 (windowLog), 201 (checksum)."""
    L = libzstd()
    L.ZSTD_createCCtx.restype = C.c_void_p
    L.ZSTD_freeCCtx.argtypes = [C.c_void_p]
    L.ZSTD_CCtx_setParameter.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ZSTD_CCtx_setParameter.restype = C.c_size_t
    L.ZSTD_compress2.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.ZSTD_compress2.restype = C.c_size_t
    ctx = C.c_void_p(L.ZSTD_createCCtx())
    try:
        for par, val in ((100, level), (101, window_log), (201, int(checksum))):
            if val:
                assert not L.ZSTD_isError(L.ZSTD_CCtx_setParameter(ctx, par, val))
        cap = L.ZSTD_compressBound(len(data))
        out = C.create_string_buffer(max(1, cap))
        n = L.ZSTD_compress2(ctx, out, cap, data, len(data))
        assert not L.ZSTD_isError(n)
        return out.raw[:n]
    finally:
        L.ZSTD_freeCCtx(ctx)


class _ZBuf(C.Structure):
    _fields_ = [("p", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]


def block_regen_sizes(frame: bytes, info: dict, nbytes: int):
    """The bytes each block of a valid frame regenerates, by libzstd's streaming
    decoder fed one block at a time (it decodes a block when its last byte is
    in); and the decoded bytes."""
    L = libzstd()
    L.ZSTD_createDStream.restype = C.c_void_p
    L.ZSTD_freeDStream.argtypes = [C.c_void_p]
    L.ZSTD_initDStream.argtypes = [C.c_void_p]
    L.ZSTD_initDStream.restype = C.c_size_t
    L.ZSTD_decompressStream.argtypes = [C.c_void_p, C.POINTER(_ZBuf), C.POINTER(_ZBuf)]
    L.ZSTD_decompressStream.restype = C.c_size_t
    zds = C.c_void_p(L.ZSTD_createDStream())
    try:
        assert not L.ZSTD_isError(L.ZSTD_initDStream(zds))
        src = C.create_string_buffer(bytes(frame), len(frame))
        dst = C.create_string_buffer(max(1, nbytes))
        out = _ZBuf(C.addressof(dst), nbytes, 0)
        inp = _ZBuf(C.addressof(src), 0, 0)
        sizes = []
        ends = [b["pos"] + 3 + (1 if b["type"] == "rle" else b["size"]) for b in info["blocks"]]
        for end in ends:
            inp.size = end
            before = out.pos
            r = L.ZSTD_decompressStream(zds, C.byref(out), C.byref(inp))
            assert not L.ZSTD_isError(r), r
            assert inp.pos == end
            sizes.append(out.pos - before)
        assert r == 0, "the frame is not finished at its last block"
        return sizes, dst.raw[:out.pos]
    finally:
        L.ZSTD_freeDStream(zds)


# ---- inspector -------------------------------------------------------------------
def _lit_header(b: bytes, p: int):
    """(type, streams, regenerated, compressed or None, header bytes) at b[p]."""
    b0 = b[p]
    t, sf = b0 & 3, (b0 >> 2) & 3
    if t < 2:
        if sf in (0, 2):
            return t, 1, b0 >> 3, None, 1
        if sf == 1:
            return t, 1, (b0 >> 4) | b[p + 1] << 4, None, 2
        return t, 1, (b0 >> 4) | b[p + 1] << 4 | b[p + 2] << 12, None, 3
    hdr = 3 if sf < 2 else sf + 2
    bits = 10 if sf < 2 else 14 if sf == 2 else 18
    v = int.from_bytes(b[p:p + hdr], "little") >> 4
    return t, 1 if sf == 0 else 4, v & ((1 << bits) - 1), (v >> bits) & ((1 << bits) - 1), hdr


MAX_LOG = (9, 8, 9)        # literal lengths, offsets, match lengths
MAX_SYMBOLS = (36, 32, 53)


def read_ncount(buf: bytes, pos: int, max_log: int):
    """An FSE table description at buf[pos] (RFC 8878 4.1.1): (normalised counts
    with -1 for "less than 1", accuracy log, bytes used)."""
    acc = int.from_bytes(buf[pos:pos + 512], "little")
    have = 8 * len(buf[pos:pos + 512])
    at = 0

    def read(n):
        nonlocal at
        v = (acc >> at) & ((1 << n) - 1)
        at += n
        return v

    log = 5 + read(4)
    assert log <= max_log, (log, max_log)
    remaining = 1 << log
    norm = []
    while remaining > 0:
        width = (remaining + 1).bit_length()
        low_mask = (1 << (width - 1)) - 1
        small = (1 << width) - 1 - (remaining + 1)   # values below it take width - 1 bits
        v = (acc >> at) & ((1 << width) - 1)
        if (v & low_mask) < small:
            v &= low_mask
            at += width - 1
        else:
            at += width
            if v > low_mask:
                v -= small
        p = v - 1
        remaining -= abs(p)
        assert remaining >= 0, "probabilities exceed the table"
        norm.append(p)
        if p == 0:
            while True:
                r = read(2)
                norm += [0] * r
                if r != 3:
                    break
        assert len(norm) <= 256
    assert at <= have, "description runs past the buffer"
    return norm, log, (at + 7) // 8


def _zero_repeat(norm):
    """The longest count of zero probabilities a description's repeat flags
    carry: a run of zeros less its first (which is coded as a value)."""
    best = run = 0
    for c in norm:
        run = run + 1 if c == 0 else 0
        best = max(best, run)
    return max(0, best - 1)


def frame_header(frame: bytes):
    """The frame-header features alone (info["blocks"] empty)."""
    return inspect(frame, blocks=False)


def inspect(frame: bytes, blocks: bool = True):
    """Frame-header features and, per block, type / size and (compressed blocks)
    the literals type, stream count, weight coding, sequence count and table
    modes, with the positions the mutations patch; of a block that describes
    sequence tables, each table as read_ncount reads it ("tables"), and where all
    three are FSE_Compressed their accuracy logs ("table_logs"), whether a
    probability is -1 ("minus1") and the longest zero run the repeat flags carry
    ("zero_repeat")."""
    f = bytes(frame)
    assert struct.unpack_from("<I", f, 0)[0] == MAGIC
    d = f[4]
    single, fcs_flag, did_flag = (d >> 5) & 1, d >> 6, d & 3
    pos = 5
    window = None
    if not single:
        window = f[pos]
        pos += 1
    did_bytes = (0, 1, 2, 4)[did_flag]
    did_pos = pos
    pos += did_bytes
    fcs_bytes = (single, 2, 4, 8)[fcs_flag]
    fcs = None
    if fcs_bytes:
        fcs = int.from_bytes(f[pos:pos + fcs_bytes], "little") + (256 if fcs_bytes == 2 else 0)
    info = dict(single_segment=bool(single), window=window, dict_id_bytes=did_bytes,
                dict_id_pos=did_pos, fcs_bytes=fcs_bytes, fcs_pos=pos, fcs=fcs,
                checksum=bool(d & 4), blocks=[])
    pos += fcs_bytes
    info["header_bytes"] = pos
    if not blocks:
        return info
    while True:
        bh = int.from_bytes(f[pos:pos + 3], "little")
        last, btype, size = bh & 1, (bh >> 1) & 3, bh >> 3
        blk = dict(pos=pos, type=("raw", "rle", "compressed", "reserved")[btype], size=size,
                   last=bool(last))
        body = pos + 3
        if btype == 2:
            t, ns, regen, comp, hdr = _lit_header(f, body)
            blk.update(lit_pos=body, lit_type=LIT_TYPES[t], lit_streams=ns, lit_regen=regen,
                       lit_comp=comp, lit_hdr=hdr, weights=None)
            if t == 2:
                blk["tree_pos"] = body + hdr
                blk["weights"] = "direct" if f[body + hdr] >= 128 else "fse"
            sp = body + hdr + (regen if t == 0 else 1 if t == 1 else comp)
            blk["seq_pos"] = sp
            n = f[sp]
            cb = 1
            if n == 255:
                n, cb = f[sp + 1] + (f[sp + 2] << 8) + 0x7F00, 3
            elif n >= 128:
                n, cb = ((n - 128) << 8) + f[sp + 1], 2
            blk["nseq"] = n
            blk["modes"] = None
            if n:
                m = f[sp + cb]
                blk["modes"] = (MODES[m >> 6], MODES[(m >> 4) & 3], MODES[(m >> 2) & 3])
                blk["tables_pos"] = tp = sp + cb + 1
                # the descriptions, in the order LL, OF, ML: FSE_Compressed tables
                # are read, an RLE table is its one symbol
                blk["tables"] = []
                for k, mode in enumerate(blk["modes"]):
                    tab = None
                    if mode == "fse":
                        norm, log, used = read_ncount(f[:body + size], tp, MAX_LOG[k])
                        assert len(norm) <= MAX_SYMBOLS[k], (k, len(norm))
                        tab = dict(norm=norm, log=log, nbytes=used, minus1=-1 in norm,
                                   zero_repeat=_zero_repeat(norm))
                        tp += used
                    elif mode == "rle":
                        tp += 1
                    blk["tables"].append(tab)
                blk["tables_end"] = tp
                if blk["modes"] == ("fse", "fse", "fse"):
                    blk["table_logs"] = tuple(t["log"] for t in blk["tables"])
                    blk["minus1"] = any(t["minus1"] for t in blk["tables"])
                    blk["zero_repeat"] = max(t["zero_repeat"] for t in blk["tables"])
        info["blocks"].append(blk)
        pos = body + (1 if btype == 1 else size)
        if last:
            break
    info["end"] = pos + (4 if info["checksum"] else 0)
    assert info["end"] == len(f), (info["end"], len(f))
    return info


# ---- hand-assembler --------------------------------------------------------------
LL_NORM = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1,
           1, 1, 1, 1, -1, -1, -1, -1]
ML_NORM = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
OF_NORM = [1, 1, 1, 1, 1, 1, 2, 2, 2] + [1] * 15 + [-1] * 5
LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048,
                             4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027,
                                2051, 4099, 8195, 16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def fse_decode_table(norm, log):
    """[(symbol, bits, base)] by state (RFC 8878 4.1.1)."""
    size = 1 << log
    sym = [0] * size
    high = size - 1
    for s, c in enumerate(norm):
        if c == -1:
            sym[high] = s
            high -= 1
    step, mask, pos = (size >> 1) + (size >> 3) + 3, size - 1, 0
    for s, c in enumerate(norm):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos > high:
                pos = (pos + step) & mask
    assert pos == 0
    nxt = [1 if c == -1 else c for c in norm]
    out = []
    for u in range(size):
        s = sym[u]
        ns = nxt[s]
        nxt[s] += 1
        nb = log - (ns.bit_length() - 1)
        out.append((s, nb, (ns << nb) - size))
    return out


def _code(value, base, bits):
    c = max(i for i, b in enumerate(base) if b <= value)
    assert value - base[c] < (1 << bits[c])
    return c, value - base[c], bits[c]


def sequences_bitstream(seqs):
    """The FSE bitstream of (literal_length, match_length, offset_value) records
    coded with the predefined tables: the decoder's reads in order, written
    backwards."""
    tabs = (fse_decode_table(LL_NORM, 6), fse_decode_table(OF_NORM, 5), fse_decode_table(ML_NORM, 6))
    codes = []
    for ll, ml, ov in seqs:
        assert ov >= 1
        oc = ov.bit_length() - 1
        codes.append((_code(ll, LL_BASE, LL_BITS), (oc, ov - (1 << oc), oc), _code(ml, ML_BASE, ML_BITS)))
    # states, last sequence first: any state of the symbol, then the state of
    # the symbol whose transition reaches the next one
    n = len(seqs)
    states = [[0, 0, 0] for _ in range(n)]
    upd = [[(0, 0)] * 3 for _ in range(n)]
    for k in range(3):
        tab = tabs[k]
        for i in range(n - 1, -1, -1):
            c = codes[i][k][0]
            if i == n - 1:
                states[i][k] = next(u for u, (s, _, _) in enumerate(tab) if s == c)
            else:
                tgt = states[i + 1][k]
                u = next(u for u, (s, nb, base) in enumerate(tab)
                         if s == c and base <= tgt < base + (1 << nb))
                states[i][k] = u
                upd[i][k] = (tgt - tab[u][2], tab[u][1])
    reads = [(states[0][0], 6), (states[0][1], 5), (states[0][2], 6)]
    for i in range(n):
        (_, le, lb), (_, oe, ob), (_, me, mb) = codes[i]
        reads += [(oe, ob), (me, mb), (le, lb)]
        if i + 1 < n:
            reads += [upd[i][0], upd[i][2], upd[i][1]]
    acc = 1
    for v, nb in reads:
        assert 0 <= v < (1 << nb) or nb == 0 and v == 0
        acc = (acc << nb) | v
    return acc.to_bytes((acc.bit_length() + 7) // 8, "little")


def _raw_rle_lit_header(t, regen):
    if regen < 32:
        return bytes([t | regen << 3])
    if regen < 4096:
        return struct.pack("<H", t | 1 << 2 | regen << 4)
    return (t | 3 << 2 | regen << 4).to_bytes(3, "little")


def compressed_block(literals, seqs):
    """Block content: Raw literals (bytes) or RLE literals ((byte, count)), then the
    sequences with the predefined tables."""
    if isinstance(literals, tuple):
        byte, count = literals
        out = _raw_rle_lit_header(1, count) + bytes([byte])
    else:
        out = _raw_rle_lit_header(0, len(literals)) + bytes(literals)
    n = len(seqs)
    if n < 128:
        out += bytes([n])
    elif n < 0x7F00:
        out += bytes([(n >> 8) + 128, n & 255])
    else:
        out += b"\xff" + struct.pack("<H", n - 0x7F00)
    if n:
        out += b"\x00" + sequences_bitstream(seqs)
    return out


def assemble_frame(blocks, content_size=None):
    """blocks: ("raw", bytes) | ("rle", byte, count) | ("seq", literals, [(ll, ml, ov)])
    | ("content", bytes: a compressed block's bytes as given).  Single_Segment,
    Frame_Content_Size = content_size (default: what the blocks decode to, where
    that is known: not for "content" blocks)."""
    total = 0
    body = b""
    for i, blk in enumerate(blocks):
        last = int(i == len(blocks) - 1)
        if blk[0] == "raw":
            btype, size, data = 0, len(blk[1]), bytes(blk[1])
            total += size
        elif blk[0] == "rle":
            btype, size, data = 1, blk[2], bytes([blk[1]])
            total += size
        else:
            data = compressed_block(blk[1], blk[2]) if blk[0] == "seq" else bytes(blk[1])
            btype, size = 2, len(data)
            if blk[0] == "seq":
                lits = blk[1][1] if isinstance(blk[1], tuple) else len(blk[1])
                total += lits + sum(ml for _, ml, _ in blk[2])
        assert size <= BLOCK_MAX
        body += (size << 3 | btype << 1 | last).to_bytes(3, "little") + data
    n = total if content_size is None else content_size
    if n < 256:
        hdr = bytes([0x20, n])
    else:
        hdr = bytes([0x20 | 2 << 6]) + struct.pack("<I", n)
    return struct.pack("<I", MAGIC) + hdr + body


def assembled_valid():
    """[(name, frame, decoded length)]: frames libzstd will not emit on request."""
    lit = bytes(range(65, 65 + 26))
    out = []

    def put(name, blocks):
        fr = assemble_frame(blocks)
        out.append((name, fr, frame_header(fr)["fcs"]))

    put("raw_block", [("raw", b"hello, zstd")])
    put("rle_block", [("rle", 0x5A, 1000)])
    put("raw_rle_raw", [("raw", lit), ("rle", 7, 300), ("raw", lit[::-1])])
    put("literals_only", [("seq", lit, [])])
    put("rle_literals_only", [("seq", (0x33, 500), [])])
    put("new_offsets", [("seq", lit, [(5, 4, 3 + 2), (3, 10, 3 + 8), (0, 3, 3 + 1)])])
    put("overlapping_match", [("seq", b"ab", [(2, 200, 3 + 2), (0, 70, 3 + 1)])])
    put("rle_literals_with_matches", [("seq", (0x41, 40), [(10, 5, 3 + 3), (20, 8, 3 + 30)])])
    # repeat codes with literals: 1 -> rep0, 2 -> rep1, 3 -> rep2
    put("repeat_1_2_3", [("seq", lit, [(4, 3, 3 + 4), (2, 4, 3 + 2), (2, 5, 3 + 6),
                                       (1, 3, 1), (1, 4, 2), (1, 5, 3), (1, 6, 3), (1, 3, 2)])])
    # ... and after literal_length 0: 1 -> rep1, 2 -> rep2, 3 -> rep0 - 1
    put("repeat_ll0", [("seq", lit, [(6, 3, 3 + 5), (2, 4, 3 + 3), (2, 5, 3 + 7),
                                     (0, 3, 1), (0, 4, 2), (0, 5, 3), (1, 3, 1), (0, 6, 3)])])
    # the frame's initial repeat offsets 1, 4, 8
    put("initial_repeats", [("seq", lit, [(9, 3, 1), (1, 4, 2), (1, 5, 3), (0, 4, 3)])])
    # repeat offsets and matches carry across blocks (and over raw / RLE ones)
    put("across_blocks", [("seq", lit, [(10, 6, 3 + 7)]), ("rle", 9, 50),
                          ("seq", b"xyz", [(1, 20, 3 + 60), (1, 5, 1), (0, 4, 1)]),
                          ("raw", b"tail"), ("seq", b"", [(0, 30, 3 + 100)])])
    put("long_lengths", [("seq", bytes(range(256)) * 20, [(5000, 3000, 3 + 4000), (17, 35, 3 + 1),
                                                          (64, 131, 3 + 7000), (0, 65539, 3 + 3)])])
    # matches that reach back across blocks, farther than any on-chip window
    far = bytes((i * 7 + i // 251) & 255 for i in range(100_000))
    put("far_matches", [("raw", far), ("raw", far[::-1]),
                        ("seq", b"", [(0, 1000, 3 + 190_000), (0, 50, 3 + 170_000),
                                      (0, 300, 3 + 200_999)])])
    put("many_sequences", [("seq", lit * 40, [(1 + i % 3, 3 + i % 40, 3 + 1 + i % 5)
                                              for i in range(300)])])
    return out


def assembled_malformed():
    """[(name, frame, expected length, status)] -- sequences libzstd never writes."""
    lit = bytes(range(65, 65 + 26))
    out = []

    def put(name, blocks, status=CORRUPT, n=None):
        fr = assemble_frame(blocks, content_size=n)
        out.append((name, fr, frame_header(fr)["fcs"], status))

    put("offset_before_frame_start", [("seq", lit, [(5, 4, 3 + 6)])])
    put("offset_before_frame_start_far", [("raw", lit), ("seq", lit, [(5, 4, 3 + 32)])])
    put("offset_0", [("seq", lit, [(0, 4, 3)])])           # repeat offset 1 (= 1) minus 1
    put("match_length_past_output", [("seq", lit, [(5, 40, 3 + 2)])], n=26 + 30)
    put("literals_past_block_literals", [("seq", lit, [(27, 4, 3 + 2)])], n=26 + 4)
    put("output_one_byte_short", [("seq", lit, [(5, 4, 3 + 2)])], n=26 + 4 + 1)
    put("output_one_byte_long", [("seq", lit, [(5, 4, 3 + 2)])], n=26 + 4 - 1)
    put("sequence_count_no_bytes", [("content", _raw_rle_lit_header(0, 4) + b"abcd" + b"\x05")], n=4)
    put("sequences_without_bitstream",
        [("content", _raw_rle_lit_header(0, 4) + b"abcd" + b"\x01\x00")], n=7)
    put("sequences_bitstream_no_end_mark",
        [("content", _raw_rle_lit_header(0, 4) + b"abcd" + b"\x01\x00\x12\x34\x00")], n=7)
    put("treeless_in_first_block", [("content", bytes([0x13, 0x40, 0x00]) + b"\x01\x00")], n=1)
    put("repeat_mode_in_first_block",
        [("content", _raw_rle_lit_header(0, 4) + b"abcd" + b"\x01\xc0\x01")], n=7)
    put("reserved_sequence_mode_bits",
        [("content", _raw_rle_lit_header(0, 4) + b"abcd" + b"\x01\x01\x01")], n=7)
    put("literals_more_than_output", [("seq", lit, [])], n=20)
    put("rle_block_past_output", [("rle", 1, 100)], n=99)
    return out


# ---- named mutations of frames libzstd / c-blosc made -----------------------------
def _patched(frame, pos, data):
    b = bytearray(frame)
    b[pos:pos + len(data)] = data
    return bytes(b)


def _block_header(size, btype, last):
    return (size << 3 | btype << 1 | int(last)).to_bytes(3, "little")


def _weights_break(frame, blk):
    """A direct-weights tree description with one nibble changed so that the
    weights no longer complete to a power of two."""
    p = blk["tree_pos"]
    nw = frame[p] - 127

    def valid(ws):
        s = sum(1 << (w - 1) for w in ws if w)
        if s == 0 or any(w > 11 for w in ws):
            return False
        left = (1 << s.bit_length()) - s
        return left & (left - 1) == 0 and s.bit_length() <= 11

    ws = [(frame[p + 1 + i // 2] >> (0 if i & 1 else 4)) & 15 for i in range(nw)]
    assert valid(ws)
    for i in range(nw):
        for v in range(1, 12):
            t = list(ws)
            t[i] = v
            if not valid(t):
                byte = frame[p + 1 + i // 2]
                byte = (byte & 0xF0 | v) if i & 1 else (byte & 0x0F | v << 4)
                return _patched(frame, p + 1 + i // 2, bytes([byte]))
    raise AssertionError("no invalid weight set one nibble away")


def named_mutations(golden):
    """[(name, frame, expected length, status)] over the golden frames (a dict
    name -> (frame, nbytes)): one defect each."""
    out = []

    def put(name, src, data, status):
        out.append((f"{src}:{name}", bytes(data), golden[src][1], status))

    def first(pred, what):
        for name, (fr, _) in golden.items():
            if name.startswith("blosc_"):
                continue
            info = inspect(fr)
            for blk in info["blocks"]:
                if pred(info, blk):
                    return name, fr, info, blk
        raise AssertionError("no golden frame with " + what)

    src = "text_windowed"          # many blocks, checksum, window descriptor
    fr, _ = golden[src]
    info = inspect(fr)
    assert len(info["blocks"]) > 4 and info["checksum"] and not info["single_segment"]
    put("truncated_by_1", src, fr[:-1], CORRUPT)
    put("truncated_by_half", src, fr[:len(fr) // 2], CORRUPT)
    put("magic_wrong", src, _patched(fr, 3, b"\xfc"), BAD_HEADER)
    put("reserved_frame_header_bit", src, _patched(fr, 4, bytes([fr[4] | 8])), BAD_HEADER)
    put("fcs_not_expected", src,
        _patched(fr, info["fcs_pos"], bytes([fr[info["fcs_pos"]] ^ 1])), BAD_HEADER)
    put("skippable_magic", src, _patched(fr, 0, struct.pack("<I", 0x184D2A53)), UNSUPPORTED)
    b1 = info["blocks"][1]
    put("block_size_past_frame", src,
        _patched(fr, b1["pos"], _block_header(BLOCK_MAX, 2, False)), CORRUPT)
    put("block_size_above_128k", src,
        _patched(fr, b1["pos"], _block_header(BLOCK_MAX + 1, 2, False)), CORRUPT)
    put("reserved_block_type", src,
        _patched(fr, b1["pos"], _block_header(b1["size"], 3, False)), CORRUPT)
    put("trailing_bytes", src, fr + b"\0", CORRUPT)

    src = "text_1stream"           # Single_Segment, one block, no checksum
    fr, _ = golden[src]
    info = inspect(fr)
    assert info["single_segment"] and not info["checksum"] and len(info["blocks"]) == 1
    blk = info["blocks"][0]
    put("last_block_flag_missing", src,
        _patched(fr, blk["pos"], _block_header(blk["size"], 2, False)), CORRUPT)
    put("dictionary_id", src, fr[:4] + bytes([fr[4] | 1, 5]) + fr[5:], UNSUPPORTED)
    put("header_does_not_fit", src, fr[:5], BAD_HEADER)
    put("trailing_bytes", src, fr + b"\0", CORRUPT)
    # the literals' compressed size: the whole block and more
    assert blk["lit_type"] == "compressed" and blk["lit_hdr"] == 3
    v = int.from_bytes(fr[blk["lit_pos"]:blk["lit_pos"] + 3], "little") | 0x3FF << 14
    put("literals_size_past_block", src, _patched(fr, blk["lit_pos"], v.to_bytes(3, "little")),
        CORRUPT)

    src, fr, info, blk = first(lambda i, b: b["type"] == "compressed" and b.get("lit_streams") == 4
                               and b["lit_type"] == "compressed", "4-stream Huffman literals")
    jump = blk["tree_pos"]  # the jump table follows the tree description: found by its status
    # the tree description's size is not in the header; the jump table is the
    # last 6 bytes before the streams, which end at seq_pos.  Setting every
    # candidate would hide errors, so derive it: direct weights take
    # 1 + ceil(n / 2) bytes, FSE weights 1 + the header byte.
    hb = fr[jump]
    jump += 1 + ((hb - 127 + 1) // 2 if hb >= 128 else hb)
    put("jump_table_past_literals", src, _patched(fr, jump, b"\xff\xff"), CORRUPT)

    src, fr, info, blk = first(lambda i, b: b.get("weights") == "direct", "direct weights")
    put("huffman_weights_not_power_of_two", src, _weights_break(fr, blk), CORRUPT)

    src, fr, info, blk = first(lambda i, b: b.get("modes") and b["modes"][0] == "fse",
                               "an FSE-compressed literal-length table")
    p = blk["tables_pos"]
    put("fse_accuracy_log_too_large", src, _patched(fr, p, bytes([fr[p] | 0x0F])), CORRUPT)

    for name, fr, n, status in assembled_malformed():
        out.append((f"assembled:{name}", fr, n, status))

    # blosc-zstd: the container's and the streams' own checks
    src = "blosc_ts2_sh1_blocks"
    fr, _ = golden[src]
    h = header(fr)
    st = blosc_streams(fr)
    _, _, pos, cs, n = next(s for s in st if s[3] != s[4])
    put("csize_past_frame", src, _patched(fr, st[0][2], struct.pack("<I", h["cbytes"])), CORRUPT)
    zi = inspect(fr[pos + 4:pos + 4 + cs])
    assert zi["fcs_bytes"] and zi["fcs"] == n
    q = pos + 4 + zi["fcs_pos"]
    put("stream_declares_other_length", src, _patched(fr, q, bytes([fr[q] ^ 1])), BAD_HEADER)
    put("stream_without_zstd_magic", src, _patched(fr, pos + 4, b"\x00"), BAD_HEADER)
    put("truncated_by_1", src, fr[:-1], BAD_HEADER)
    put("compcode_zlib", src, _patched(fr, 2, bytes([(h["flags"] & 0x1f) | (3 << 5)])), UNSUPPORTED)
    return out


# ---- blosc-zstd frames built from per-stream libzstd output ---------------------------
def blosc_zstd_frame(data: bytes, ts: int, shuffle: int, blocksize: int, split: bool,
                     level: int = 3) -> bytes:
    """A blosc1 frame with the zstd codec whose blocks are split into typesize
    streams (c-blosc 1.21 and this library never split zstd blocks): shuffled by
    the oracle's shuffles, each stream one ZSTD_compress frame (stored raw when
    that does not shrink it)."""
    from codec_helpers import shuffle as shuf
    n = len(data)
    nblocks = -(-n // blocksize)
    flags = (4 << 5) | (0 if split else 0x10) | (1 if shuffle == 1 else 4 if shuffle == 2 else 0)
    body = b""
    starts = []
    base = 16 + 4 * nblocks
    for j in range(nblocks):
        blk = data[j * blocksize:(j + 1) * blocksize]
        leftover = len(blk) != blocksize
        if shuffle == 1 and ts > 1:
            blk = shuf("shuffle", ts, blk)
        elif shuffle == 2 and (len(blk) // ts) % 8 == 0:
            blk = shuf("bitshuffle", ts, blk)
        ns = ts if split and not leftover and blocksize // ts >= 128 else 1
        starts.append(base + len(body))
        slen = len(blk) // ns
        for s in range(ns):
            raw = blk[s * slen:(s + 1) * slen]
            z = zstd_compress(raw, level)
            if len(z) >= len(raw):
                z = raw
            body += struct.pack("<I", len(z)) + z
    cbytes = base + len(body)
    return (bytes([2, 1, flags, ts]) + struct.pack("<III", n, blocksize, cbytes) +
            struct.pack("<%dI" % nblocks, *starts) + body)


def load_golden():
    """{name: (frame, expected length)} and {name: sha256 of the payload}."""
    z = np.load(GOLDEN)
    frames, digests = {}, {}
    for i, name in enumerate(z["names"]):
        frames[str(name)] = (z[f"frame_{i}"].tobytes(), int(z["nbytes"][i]))
        digests[str(name)] = str(z["sha256"][i])
    return frames, digests


def reference_decode(frame: bytes, nbytes: int) -> bytes:
    """libzstd (plain frames) / the restated blosc container over libzstd."""
    from codec_helpers import blosc_zstd_decode
    if struct.unpack_from("<I", frame, 0)[0] == MAGIC:
        return zstd_decode(frame, nbytes)
    return blosc_zstd_decode(frame)


def conditions(frames):
    """The fixture's stated conditions (golden/make_zstd_frames.py asserts them when
    it writes the file, test_zstddec_cpu.py on the committed file)."""
    plain = {k: inspect(fr) for k, (fr, _) in frames.items() if not k.startswith("blosc_")}
    blocks = [(k, i, b) for k, i in plain.items() for b in i["blocks"]]
    comp = [(k, i, b) for k, i, b in blocks if b["type"] == "compressed"]

    def any_block(pred):
        return any(pred(i, b) for _, i, b in comp)

    assert any_block(lambda i, b: b["lit_type"] == "compressed" and b["lit_streams"] == 1)
    assert any_block(lambda i, b: b["lit_type"] == "compressed" and b["lit_streams"] == 4)
    assert any_block(lambda i, b: b["lit_type"] == "treeless" and b["lit_streams"] == 4)
    assert any_block(lambda i, b: b["lit_type"] == "raw")
    assert any_block(lambda i, b: b["weights"] == "direct")
    assert any_block(lambda i, b: b["weights"] == "fse")
    assert any_block(lambda i, b: b["nseq"] > 10000)
    for k in range(3):
        assert any_block(lambda i, b: b["modes"] and b["modes"][k] == "rle"), k
        assert any_block(lambda i, b: b["modes"] and b["modes"][k] == "fse"), k
        assert any_block(lambda i, b: b["modes"] and b["modes"][k] == "predefined"), k
    assert any(sum(1 for b in i["blocks"] if b.get("modes") and "fse" in b["modes"]) >= 2
               for i in plain.values())
    assert any(not i["single_segment"] and i["checksum"] and i["fcs_bytes"] == 2 and
               len(i["blocks"]) >= 30 and
               any(b.get("modes") and b["modes"][0] == "predefined" for b in i["blocks"]) and
               any(b.get("modes") and b["modes"][0] == "fse" for b in i["blocks"])
               for i in plain.values())
    # an RLE block next to a compressed one (which comes first depends on libzstd's version)
    assert any(sorted(b["type"] for b in i["blocks"][:2]) == ["compressed", "rle"]
               for i in plain.values())
    assert any(b["type"] == "raw" for _, _, b in blocks)
    assert any(i["fcs_bytes"] == 1 and i["fcs"] == 0 for i in plain.values())
    assert any(i["fcs_bytes"] == 1 and i["fcs"] == 5 for i in plain.values())
    assert {i["fcs_bytes"] for i in plain.values()} >= {1, 2, 4}
    assert any(len(i["blocks"]) >= 2 and i["fcs"] > BLOCK_MAX for i in plain.values())
    bl = {k: header(fr) for k, (fr, _) in frames.items() if k.startswith("blosc_")}
    assert all(h["flags"] >> 5 == 4 and h["version"] == 2 for h in bl.values())
    assert {h["typesize"] for h in bl.values()} >= {1, 2, 4, 8}
    assert any(h["flags"] & 0x1 for h in bl.values())
    assert any(h["flags"] & 0x4 for h in bl.values())
    assert any(not h["flags"] & 0x5 and not h["flags"] & 0x2 for h in bl.values())
    assert any(h["flags"] & 0x2 for h in bl.values())
    assert any(h["blocksize"] == 16384 and h["nbytes"] // 16384 >= 2 and h["nbytes"] % 16384
               for h in bl.values())
    assert any(h["blocksize"] > 32768 and h["blocksize"] >= h["nbytes"] and h["flags"] & 0x5
               for h in bl.values())
