"""Frames aimed at the phases of the block-parallel zstd decode
(csrc/aqz_zstdpar.hh), shared by test_zstdpar_cpu.py and test_gpu_zstdpar.py.

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import struct

from codec_helpers import zstd_decode
from zstddec_helpers import assemble_frame, frame_header, inspect, load_golden

LIT = bytes(range(65, 65 + 26))


def block_capacity(n: int) -> int:
    """Blocks the block table of a chunk of n bytes holds (zpar::block_capacity)."""
    return n // 1024 + 16


def parallel_scratch_bytes(n: int, chunks: int) -> int:
    """What AQZ_DECODE_ZSTD_PARALLEL adds to aqz_decompressor_scratch_bytes_for, as
    include/aqz_gpu.h documents it."""
    def r16(v):
        return (v + 15) & ~15
    return chunks * (64 * (n // 1024 + 16) + r16(n) + r16(12 * (n // 3))) + r16(8 * chunks) + 16


def definers(info):
    """Per compressed block of an inspected frame: the index of the block that
    defines the Huffman tree and the LL / OF / ML table in effect (None: the block
    does not use one)."""
    last = [None] * 4
    out = {}
    for j, b in enumerate(info["blocks"]):
        if b["type"] != "compressed":
            continue
        use = [None] * 4
        if b["lit_type"] == "compressed":
            last[0] = j
        if b["lit_type"] in ("compressed", "treeless"):
            use[0] = last[0]
        if b["nseq"]:
            for k, mode in enumerate(b["modes"]):
                if mode != "repeat":
                    last[1 + k] = j
                use[1 + k] = last[1 + k]
        out[j] = use
    return out


def _block_header(size, btype, last):
    return (size << 3 | btype << 1 | int(last)).to_bytes(3, "little")


def chained_with_raw_between():
    """Blocks 0 and 1 of the golden text_windowed frame (1: treeless, its tree is
    block 0's; three FSE-described tables), a raw block, block 1 again with all
    three tables in Repeat_Mode (its descriptions cut out: the definer of every
    table lies two blocks back, the tree's three), a raw block, and block 1 with
    only the offset table in Repeat_Mode (definer four blocks back, reached by
    walking past block 1's literal-length description).  The same tables and
    bitstreams give the same lengths, so every copy regenerates what block 1 does.
    No content checksum; Frame_Content_Size patched.  (name, frame, length)."""
    from zstddec_helpers import block_regen_sizes
    frames, _ = load_golden()
    fr, n = frames["text_windowed"]
    info = inspect(fr)
    bare = bytearray(fr[:-4])                # without the checksum: the helper's streaming
    bare[4] &= ~4 & 0xff                     # decode then ends with the last block
    sizes, _ = block_regen_sizes(bytes(bare), inspect(bytes(bare)), n)
    b1 = info["blocks"][1]
    assert b1["lit_type"] == "treeless" and b1["modes"] == ("fse", "fse", "fse")
    body = b1["pos"] + 3
    content = fr[body:body + b1["size"]]
    tp, te = b1["tables_pos"] - body, b1["tables_end"] - body
    ll_end = tp + b1["tables"][0]["nbytes"]
    of_end = ll_end + b1["tables"][1]["nbytes"]
    all_repeat = content[:tp - 1] + b"\xfc" + content[te:]
    of_repeat = content[:tp - 1] + bytes([2 << 6 | 3 << 4 | 2 << 2]) + content[tp:ll_end] + \
        content[of_end:]
    raw = b"<<a raw block between>>"
    out = bytearray(fr[:body + b1["size"]] +
                    _block_header(len(raw), 0, False) + raw +
                    _block_header(len(all_repeat), 2, False) + all_repeat +
                    _block_header(len(raw), 0, False) + raw +
                    _block_header(len(of_repeat), 2, True) + of_repeat)
    total = sizes[0] + 3 * sizes[1] + 2 * len(raw)
    out[4] &= ~4 & 0xff                      # no Content_Checksum
    assert info["fcs_bytes"] == 2
    struct.pack_into("<H", out, info["fcs_pos"], total - 256)
    out = bytes(out)
    chk = inspect(out)
    d = definers(chk)
    assert [b["type"] for b in chk["blocks"]] == ["compressed", "compressed", "raw",
                                                   "compressed", "raw", "compressed"]
    assert d[3] == [0, 1, 1, 1] and d[5] == [0, 5, 1, 5]
    return "chain_two_back", out, total


def over_capacity_frame():
    """3 blocks with content, then as many empty raw blocks as the block table of
    its chunk size holds: more blocks than the table.  (name, frame, length)."""
    blocks = [("raw", LIT), ("seq", LIT, [(5, 4, 3 + 2), (3, 10, 3 + 8)]), ("rle", 7, 100)]
    n = 26 + 26 + 14 + 100
    blocks += [("raw", b"")] * block_capacity(n)
    fr = assemble_frame(blocks)
    assert frame_header(fr)["fcs"] == n
    return "over_capacity", fr, n


def assembled_parallel():
    """[(name, frame, decoded length)]: valid frames aimed at the phases."""
    out = []

    def put(name, blocks):
        fr = assemble_frame(blocks)
        out.append((name, fr, frame_header(fr)["fcs"]))

    # record batches of 64: one short, exact, one over, two and one over
    for n in (63, 64, 65, 129):
        put(f"nseq_{n}", [("seq", LIT * 40, [(1 + i % 3, 3 + i % 40, 3 + 1 + i % 5)
                                              for i in range(n)])])
    # every match reads what the one before it wrote
    put("batch_all_dependent", [("seq", b"xy", [(2, 5, 3 + 1)] +
                                 [(0, 4 + i % 3, 3 + 1 + i % 2) for i in range(80)])])
    # no match of the batch reads another's bytes: all sources lie in the raw block
    far = bytes((i * 13 + i // 200) & 255 for i in range(4000))
    put("batch_none_dependent", [("raw", far), ("seq", LIT * 3, [(1, 8, 3 + 3000)] * 64)])
    # repeat codes as the first sequence of a block, after each kind of block
    first = ("seq", LIT * 2, [(20, 4, 3 + 5), (2, 4, 3 + 9), (2, 4, 3 + 13)])
    between = {"compressed": [], "raw": [("raw", b"0123456789")], "rle": [("rle", 0x2e, 33)]}
    for prev, mid in between.items():
        for code in (1, 2, 3):
            for ll in (2, 0):
                put(f"rep{code}_ll{ll}_after_{prev}",
                    [first] + mid + [("seq", LIT, [(ll, 5, code), (1, 3, 1), (0, 4, 2)])])
    out.append(chained_with_raw_between())
    return out


def expected_bytes(frame: bytes, n: int) -> bytes:
    return zstd_decode(frame, n)
