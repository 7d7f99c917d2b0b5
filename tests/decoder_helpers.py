"""Helpers of the blosc1-LZ4 decoder tests (test_decoder_cpu.py, test_gpu_decode.py,
golden/make_cblosc_frames.py): a restatement of the frame layout that lists a
frame's streams and LZ4 sequences, the named mutations with the status each must
get, the seeded single-byte mutations, the golden fixture's loader and the corpus
file tests/sanitize/lz4dec_sanitize.cpp reads.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import hashlib
import os
import struct

import numpy as np

from codec_helpers import header

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "cblosc_lz4_frames.npz")

OK, SKIPPED, BAD_HEADER, CORRUPT, UNSUPPORTED = range(5)

# golden frames the named mutations are applied to: a block that decodes in
# LDS, a bit-shuffled one, and one with 256 KiB streams (the scratch path)
MUTATED = ("camera_ts4_sh1", "camera_ts8_sh2", "long_streams")


def load_golden():
    """[(name, frame bytes, typesize, shuffle, sha256 hex of the payload)]"""
    z = np.load(GOLDEN)
    out = []
    for i, name in enumerate(z["names"]):
        out.append((str(name), z[f"frame_{i}"].tobytes(), int(z["typesize"][i]),
                    int(z["shuffle"][i]), str(z["sha256"][i])))
    return out


def streams(frame: bytes):
    """[(block, stream, record pos, csize, stream length)] of a non-memcpyed frame."""
    h = header(frame)
    nbytes, bs, ts, fl = h["nbytes"], h["blocksize"], h["typesize"], h["flags"]
    nblocks = -(-nbytes // bs)
    out = []
    for j in range(nblocks):
        blen = min(bs, nbytes - j * bs)
        leftover = blen != bs
        split = not (fl & 0x10) and ts <= 16 and bs // ts >= 128 and not leftover
        ns = ts if split else 1
        pos = struct.unpack_from("<I", frame, 16 + 4 * j)[0]
        for s in range(ns):
            cs = struct.unpack_from("<I", frame, pos)[0]
            out.append((j, s, pos, cs, blen // ns))
            pos += 4 + cs
    return out


def props(frame: bytes):
    """What the fixture's conditions are stated in."""
    h = header(frame)
    p = dict(flags=h["flags"], typesize=h["typesize"], memcpyed=bool(h["flags"] & 0x2),
             dont_split=bool(h["flags"] & 0x10), split_full_blocks=0, leftover=False,
             raw_stream=False, max_stream=0)
    if p["memcpyed"]:
        return p
    st = streams(frame)
    nfull = h["nbytes"] // h["blocksize"]
    p["leftover"] = h["nbytes"] % h["blocksize"] != 0
    if any(s > 0 for _, s, _, _, _ in st):
        p["split_full_blocks"] = nfull
    p["raw_stream"] = any(cs == n for _, _, _, cs, n in st)
    p["max_stream"] = max(n for *_, n in st)
    return p


def lz4_sequences(stream: bytes):
    """[(token pos, literal length, offset pos or None, match length)] of an LZ4 block."""
    p, out = 0, []
    n = len(stream)
    while True:
        t = p
        tok = stream[p]
        p += 1
        ll = tok >> 4
        if ll == 15:
            while True:
                b = stream[p]
                p += 1
                ll += b
                if b != 255:
                    break
        p += ll
        if p == n:
            out.append((t, ll, None, 0))
            return out
        op = p
        p += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = stream[p]
                p += 1
                ml += b
                if b != 255:
                    break
        out.append((t, ll, op, ml + 4))


def _first_lz4_stream(frame: bytes):
    for _, _, pos, cs, n in streams(frame):
        if cs != n:
            seq = lz4_sequences(frame[pos + 4:pos + 4 + cs])
            if len(seq) >= 2:
                return pos + 4, cs, seq
    raise AssertionError("no LZ4-compressed stream with a match in this frame")


def named_mutations(frame: bytes):
    """[(name, frame, chunk_bytes, status)] -- one defect each, on a non-memcpyed
    golden frame with at least one LZ4 stream that holds a match."""
    h = header(frame)
    nb, cb = h["nbytes"], h["cbytes"]
    assert cb == len(frame) and not h["flags"] & 0x2
    out = []

    def put(name, data, status, chunk_bytes=nb):
        out.append((name, bytes(data), chunk_bytes, status))

    def patched(pos, data):
        b = bytearray(frame)
        b[pos:pos + len(data)] = data
        return b

    put("truncated_by_1", frame[:-1], BAD_HEADER)
    put("truncated_by_half", frame[:len(frame) // 2], BAD_HEADER)
    put("cbytes_wrong", patched(12, struct.pack("<I", cb + 1)), BAD_HEADER)
    put("nbytes_not_chunk_bytes", patched(4, struct.pack("<I", nb + h["typesize"])), BAD_HEADER)
    put("version_wrong", patched(0, b"\x03"), BAD_HEADER)
    nblocks = -(-nb // h["blocksize"])
    put("bstart_past_frame", patched(16 + 4 * (nblocks - 1), struct.pack("<I", cb + 100)),
        BAD_HEADER)
    first = streams(frame)[0]
    put("csize_past_frame", patched(first[2], struct.pack("<I", cb)), CORRUPT)
    s0, cs, seq = _first_lz4_stream(frame)
    t, ll, op, ml = seq[0]
    assert op is not None and ll < 65535
    put("match_offset_0", patched(s0 + op, b"\x00\x00"), CORRUPT)
    put("match_offset_before_stream", patched(s0 + op, b"\xff\xff"), CORRUPT)
    # the last sequence (literals only): one literal more than the stream holds
    t, ll, _, _ = seq[-1]
    if ll < 15:
        lit = patched(s0 + t, bytes([frame[s0 + t] + 0x10]))
    else:
        ext = s0 + t + 1 + (ll - 15) // 255  # the last length byte (< 255)
        lit = patched(ext, bytes([frame[ext] + 1]))
    put("literal_run_past_stream", lit, CORRUPT)
    # the last match whose length field can grow in place (the token's nibble
    # below 14 -> 14, or a last length byte below 254 -> 254): the stream then
    # decodes to more bytes than the output has
    mat = None
    for t, _, op, ml in reversed(seq):
        if op is None:
            continue
        nib = frame[s0 + t] & 15
        ext = s0 + op + 2 + (ml - 4 - 15) // 255
        if nib < 14:
            mat = patched(s0 + t, bytes([frame[s0 + t] & 0xf0 | 14]))
        elif nib == 15 and frame[ext] < 254:
            mat = patched(ext, b"\xfe")
        if mat is not None:
            break
    assert mat is not None
    put("match_length_past_output", mat, CORRUPT)
    put("compcode_zstd", patched(2, bytes([(h["flags"] & 0x1f) | (4 << 5)])), UNSUPPORTED)
    return out


def byte_mutations(frame: bytes, seed: int, count: int = 200):
    """`count` seeded copies of the frame with one byte changed each."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        pos = int(rng.integers(0, len(frame)))
        b = bytearray(frame)
        b[pos] ^= int(rng.integers(1, 256))
        out.append((pos, bytes(b)))
    return out


def sha256(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def write_corpus(path, records):
    """records: (name, frame, chunk_bytes, status or -1, expected bytes or b'')."""
    with open(path, "wb") as f:
        f.write(b"AQZC" + struct.pack("<I", len(records)))
        for name, frame, chunk_bytes, status, want in records:
            nm = name.encode()
            f.write(struct.pack("<I", len(nm)) + nm)
            f.write(struct.pack("<iQI", status, chunk_bytes, len(frame)) + frame)
            f.write(struct.pack("<I", len(want)) + want)
