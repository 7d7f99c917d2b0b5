"""Every emission path of the device zstd encoder (aqz_codec.hip zstd_far,
zstd_parse, zstd_table, zstd_encode, zstd_seqtab, zstd_seqenc, zstd_segment,
zstd_chunk, zstd_write) against libzstd: the payload family of
encoder_payloads.py, stacked as the chunks of one run of gpu.Compressor, at the
sizes that sit on the encoder's edges -- the 4 KiB parse units and 8 KiB
blocks, the 64-literal Huffman floor, the Huffman groups of 8 and 32 blocks,
the 64 blocks of a zstd_seqenc / zstd_segment wave step, the aligned and
byte-wise loads of zstd_parse, the 4-byte gate of the far pass, the
Frame_Content_Size widths, the sequence-count header at 128 and the largest
match distance.

Of every frame: libzstd (and for blosc-zstd the restated container and c-blosc)
decodes it to the chunk exactly; the frame is well formed as zstddec_helpers
.inspect reads it (single segment, Frame_Content_Size = the chunk, blocks of at
most 8 KiB, nothing after the last block); it is no longer than raw blocks
would be (the encoder compresses a block only when that is smaller: 3 bytes of
header per 8 KiB block over the payload), the offsets are monotone and within
aqz_compressor_max_bytes; and the device decoder returns the same bytes.

test_device_encoder_census names, for each feature of the format the encoder
emits, a payload, size and level whose frame shows it, and asserts that no
frame of the family shows a feature outside that list.  The same family goes
through the blosc-LZ4 compressor (literal and match lengths on LZ4's 15 and
15 + 255 extension bytes, matches that end at the last byte)."""
import functools

import numpy as np
import pytest

import encoder_payloads as ep
from codec_helpers import (blosc_zstd_decode, header, libblosc, libblosc_decode, libzstd,
                           zstd_decode)
from oracle_bindings import MEAN, SPACE, TIME, U16
from test_gpu_codec import check_frames, compress_device
from test_gpu_decode import round_trip as lz4_round_trip
from test_gpu_decode import run_decoder
from zstddec_helpers import OK, block_regen_sizes, blosc_streams, inspect

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(libzstd() is None, reason="no libzstd to decode with")]

KBLOCK = 8192            # zstd::kBlock
SEED = 11
PLAIN_LEVELS = (1, 3, 9)  # no far pass, 4 far slices, 8 far slices
# parse units and blocks; the Huffman floor; Frame_Content_Size at 256 and 65792;
# 40000 / 40002: the far gate (segments of a multiple of 4 bytes) on and off; the
# 32nd / 33rd block (a second Huffman group); the 64th and 66th block of a segment
PLAIN_SIZES = (1, 2, 63, 64, 65, 255, 256, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 40000, 40002,
               65791, 65792, 262144, 262145, 270336 + 63, 524288, 524288 + 8192 + 5)
ALIGN_SIZES = (4096, 8193, 65792)
ALIGNMENTS = ((0, 0), (4, 4), (1, 1), (0, 16))   # (source base offset, pitch pad)
BLOSC_SIZES = ("one", "16ts-ts", "bs-ts", "bs", "bs+ts", "2bs+8192+ts")


def _torch():
    import torch
    return torch


@functools.lru_cache(maxsize=4)
def family(nbytes: int, names=ep.NAMES) -> np.ndarray:
    """Every kind as one chunk of nbytes; made once per size, read-only."""
    a = ep.stack(nbytes, SEED, names)
    a.setflags(write=False)
    return a


class Run:
    pass


def compress(gpu, chunks: np.ndarray, ts, codec, clevel, shuffle, base=0, pad=0):
    """The device compressor over chunks laid at base + i * (nbytes + pad) of a
    device buffer; the frames stay on the device (fr, cap, off) and come back
    (frames, offsets)."""
    torch = _torch()
    n, nb = chunks.shape
    pitch = nb + pad
    buf = torch.zeros(base + n * pitch + 64, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[base:base + n * pitch].view(n, pitch)[:, :nb] = torch.from_numpy(np.array(chunks)).to("cuda")
    comp = gpu.Compressor(nb, ts, codec=codec, clevel=clevel, shuffle=shuffle)
    r = Run()
    r.cap = comp.max_bytes(n)
    r.fr = torch.empty(r.cap, dtype=torch.uint8, device="cuda")
    r.off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    comp.run_ptr(buf.data_ptr() + base, pitch, n, r.fr.data_ptr(), r.cap, r.off.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    r.blocksize = comp.blocksize if codec == gpu.CODEC_BLOSC_ZSTD else None
    comp.close()
    r.offsets = r.off.cpu().numpy()
    f = r.fr.cpu().numpy()
    r.frames = [f[r.offsets[i]:r.offsets[i + 1]].tobytes() for i in range(n)]
    return r


def frame_header_bytes(nb):
    return 5 + (1 if nb < 256 else 2 if nb < 65536 + 256 else 4)


def check_offsets(gpu, r, n, nb, what):
    o = r.offsets
    assert o[0] == 0 and (np.diff(o) >= 0).all(), (what, o)
    assert int(o[-1]) <= gpu.lib().aqz_compressor_max_bytes(nb, n) == r.cap, (what, o[-1], r.cap)


def check_device_decoder(gpu, r, chunks, what, pad=7):
    n, nb = chunks.shape
    dec = gpu.Decompressor(nb, n, codecs=gpu.DECODE_CODEC_ZSTD)
    got = run_decoder(gpu, dec, r.fr, r.cap, r.off, n, nb, pad)
    dec.close()
    assert (got.status == OK).all(), (what, got.status)
    for i in range(n):
        assert np.array_equal(got.chunks[i], chunks[i]), (what, i)
    assert got.pads_untouched, what


def check_plain_frame(fr: bytes, data: bytes, what):
    """(a) libzstd's bytes, (b) the frame's form, (c) its size; the inspection."""
    nb = len(data)
    assert zstd_decode(fr, nb) == data, what
    info = inspect(fr)          # ends exactly at the frame's length, or asserts
    assert info["single_segment"] and info["fcs"] == nb and not info["checksum"], (what, info)
    assert info["dict_id_bytes"] == 0 and info["header_bytes"] == frame_header_bytes(nb), what
    nblk = max(1, -(-nb // KBLOCK))
    assert len(info["blocks"]) == nblk, (what, len(info["blocks"]))
    sizes, streamed = block_regen_sizes(fr, info, nb)
    assert streamed == data, what
    assert max(sizes) <= KBLOCK and sum(sizes) == nb, (what, sizes)
    assert len(fr) <= frame_header_bytes(nb) + nb + 3 * nblk, (what, len(fr))
    for b in info["blocks"]:
        if b["type"] != "rle":   # a block is compressed only when smaller than raw
            assert b["size"] <= KBLOCK, (what, b)
    return info


def check_plain_run(gpu, chunks, level, names, base=0, pad=0, what=()):
    n, nb = chunks.shape
    r = compress(gpu, chunks, 1, gpu.CODEC_ZSTD, level, 0, base, pad)
    infos = []
    for i, fr in enumerate(r.frames):
        infos.append(check_plain_frame(fr, chunks[i].tobytes(), what + (names[i], nb, level)))
    check_offsets(gpu, r, n, nb, what + (nb, level))
    check_device_decoder(gpu, r, chunks, what + (nb, level))
    return infos


# ---- what a frame shows ------------------------------------------------------------
EMITTED = {"block_raw", "block_rle", "block_compressed", "lit_raw", "huf4_direct", "huf4_fse",
           "treeless", "second_tree", "nseq_0", "nseq_1_127", "nseq_ge_128", "modes_predefined",
           "modes_fse", "modes_repeat_after_fse", "raw_between_fse_and_repeat", "minus1",
           "zero_repeat_ge_24", "zero_repeat_3_23", "sequences_at_block_ge_64", "fcs_1", "fcs_2",
           "fcs_4"}


def features(info) -> set:
    """The features of EMITTED a frame shows, the accuracy logs of its fitted
    tables as "logs_LL_OF_ML", and anything else under its own name."""
    out = {"fcs_%d" % info["fcs_bytes"]}
    if not info["single_segment"] or info["checksum"] or info["dict_id_bytes"]:
        out.add("frame_header_other")
    trees = 0
    fse_at = None
    raw_since_fse = False
    for k, b in enumerate(info["blocks"]):
        out.add("block_" + b["type"])
        if b["type"] == "raw" and fse_at is not None:
            raw_since_fse = True
        if b["type"] != "compressed":
            continue
        lt = b["lit_type"]
        if lt == "raw":
            out.add("lit_raw")
        elif lt == "rle":
            out.add("lit_rle")
        elif b["lit_streams"] != 4:
            out.add("huffman_1_stream")
        elif lt == "compressed":
            out.add("huf4_" + b["weights"])
            trees += 1
        else:
            out.add("treeless")
        n = b["nseq"]
        out.add("nseq_0" if n == 0 else "nseq_1_127" if n < 128 else
                "nseq_ge_128" if n < 0x7F00 else "nseq_3_bytes")
        if n == 0:
            continue
        if k >= 64:
            out.add("sequences_at_block_ge_64")
        m = b["modes"]
        if m == ("predefined",) * 3:
            out.add("modes_predefined")
        elif m == ("fse",) * 3:
            out.add("modes_fse")
            out.add("logs_%d_%d_%d" % b["table_logs"])
            if b["minus1"]:
                out.add("minus1")
            if b["zero_repeat"] >= 24:
                out.add("zero_repeat_ge_24")
            if any(3 <= t["zero_repeat"] <= 23 for t in b["tables"]):
                out.add("zero_repeat_3_23")
            out.add("second_fse_block" if fse_at is not None else "modes_fse")
            fse_at = k
        elif m == ("repeat",) * 3:
            if fse_at is None:
                out.add("repeat_without_fse")
            else:
                out.add("modes_repeat_after_fse")
                if raw_since_fse:
                    out.add("raw_between_fse_and_repeat")
        else:
            out.add("modes_mixed")
    if trees >= 2:
        out.add("second_tree")
    return out


def unexpected(feats: set) -> set:
    return {f for f in feats if f not in EMITTED and not f.startswith("logs_")}


# ---- plain zstd ------------------------------------------------------------------------
@pytest.mark.parametrize("nb", PLAIN_SIZES)
@pytest.mark.parametrize("level", PLAIN_LEVELS)
def test_plain_zstd_family(gpu, level, nb):
    for info in check_plain_run(gpu, family(nb), level, ep.NAMES):
        assert not unexpected(features(info))


@pytest.mark.parametrize("base,pad", ALIGNMENTS)
@pytest.mark.parametrize("nb", ALIGN_SIZES)
def test_plain_zstd_alignment(gpu, nb, base, pad):
    """A 16-byte aligned source takes zstd_parse's whole-unit loads, any other
    its dword or byte loads; off a 4-byte aligned base or pitch the far pass is
    declined (levels 3 and 9 then parse as level 1 does)."""
    for level in PLAIN_LEVELS:
        check_plain_run(gpu, family(nb), level, ep.NAMES, base, pad, what=((base, pad),))


# ---- blosc-zstd ------------------------------------------------------------------------
def blosc_size(which, ts, bs):
    return {"one": ts, "16ts-ts": 15 * ts, "bs-ts": bs - ts, "bs": bs, "bs+ts": bs + ts,
            "2bs+8192+ts": 2 * bs + 8192 + ts}[which]


@pytest.mark.parametrize("which", BLOSC_SIZES)
@pytest.mark.parametrize("clevel", [1, 5, 7])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
@pytest.mark.parametrize("ts", [1, 2, 4, 8])
def test_blosc_zstd_family(gpu, ts, shuffle, clevel, which):
    """clevel 7 makes a bit plane the Huffman group under bitshuffle; clevel >= 2
    with bitshuffle turns the far pass on.  The sizes follow the compressor's
    own block size: one element, less than 16 elements, a block less one
    element, a block, a block and one element, two blocks and a part."""
    probe = gpu.Compressor(1 << 20, ts, codec=gpu.CODEC_BLOSC_ZSTD, clevel=clevel, shuffle=shuffle)
    bs = probe.blocksize
    probe.close()
    assert bs % ts == 0 and bs >= 16 * ts
    nb = blosc_size(which, ts, bs)
    chunks = family(nb)
    n = len(chunks)
    r = compress(gpu, chunks, ts, gpu.CODEC_BLOSC_ZSTD, clevel, shuffle)
    assert r.blocksize == min(bs, nb)
    for i, fr in enumerate(r.frames):
        what = (ep.NAMES[i], nb, ts, shuffle, clevel)
        data = chunks[i].tobytes()
        h = header(fr)
        assert h["version"] == 2 and h["flags"] >> 5 == 4 and h["typesize"] == ts, what
        assert h["nbytes"] == nb and h["cbytes"] == len(fr) and len(fr) <= nb + 16, (what, h)
        assert blosc_zstd_decode(fr) == data, what
        if libblosc() is not None:
            assert libblosc_decode(fr) == data, what
        if h["flags"] & 0x2:
            continue
        assert bool(h["flags"] & 0x1) == (shuffle == 1) and bool(h["flags"] & 0x4) == (shuffle == 2)
        for _, _, pos, cs, slen in blosc_streams(fr):
            if cs == slen:
                continue     # the record stored raw
            info = inspect(fr[pos + 4:pos + 4 + cs])
            assert info["single_segment"] and info["fcs"] == slen, what
            assert cs < slen and not unexpected(features(info)), (what, features(info))
    check_offsets(gpu, r, n, nb, (nb, ts, shuffle, clevel))
    check_device_decoder(gpu, r, chunks, (nb, ts, shuffle, clevel))


@pytest.mark.parametrize("shuffle", [1, 2])
@pytest.mark.parametrize("ts", [2, 4])
def test_blosc_zstd_bytes_after_the_last_element(gpu, ts, shuffle):
    """A chunk that is no whole number of elements: its last block is 64 (a
    multiple of 8) elements and ts - 1 bytes.  c-blosc's decoder un-shuffles the
    elements and copies the bytes after them.  (Regression, found by
    test_blosc_lz4_family at typesize 2, bitshuffle, 70001 bytes: the device
    left such a block unshuffled under bitshuffle and c-blosc decoded the frame
    to other bytes.)"""
    probe = gpu.Compressor(1 << 20, ts, codec=gpu.CODEC_BLOSC_ZSTD, clevel=5, shuffle=shuffle)
    bs = probe.blocksize
    probe.close()
    nb = bs + 64 * ts + ts - 1
    names = ("dim", "camera", "text", "run_ladder", "random")
    chunks = np.array(family(nb, names))
    r = compress(gpu, chunks, ts, gpu.CODEC_BLOSC_ZSTD, 5, shuffle)
    stored = 0
    for i, fr in enumerate(r.frames):
        data = chunks[i].tobytes()
        h = header(fr)
        assert h["nbytes"] == nb and h["blocksize"] == bs and len(fr) <= nb + 16, (names[i], h)
        stored += bool(h["flags"] & 0x2)
        assert blosc_zstd_decode(fr) == data, names[i]
        if libblosc() is not None:
            assert libblosc_decode(fr) == data, names[i]
    assert stored < len(names)
    check_offsets(gpu, r, len(names), nb, (nb, ts, shuffle))
    check_device_decoder(gpu, r, chunks, (nb, ts, shuffle))


# ---- census ----------------------------------------------------------------------------
# feature -> (payload kind, chunk bytes, plain zstd level): the smallest frame of
# the family found to show it on an MI355X
WITNESS = {
    "block_raw": ("random", 2, 1),
    "block_rle": ("zeros", 1, 1),
    "block_compressed": ("dim", 64, 1),
    "lit_raw": ("literal_ladder", 255, 1),
    "huf4_direct": ("nibble_uniform", 64, 1),
    "huf4_fse": ("dim", 64, 1),
    "treeless": ("dim", 12289, 1),
    # 262145 bytes span two Huffman groups, but the second holds one byte (a raw
    # block): the smallest size of the family with a second tree is 270399
    "second_tree": ("dim", 270336 + 63, 1),
    "nseq_0": ("dim", 64, 1),
    "nseq_1_127": ("dim", 255, 1),
    "nseq_ge_128": ("dim", 4095, 1),
    "modes_predefined": ("text", 255, 1),
    "modes_fse": ("dim", 255, 1),
    "modes_repeat_after_fse": ("dim", 12289, 1),
    "raw_between_fse_and_repeat": ("raw_middle", 65791, 1),
    "minus1": ("dim", 4095, 1),
    # run lengths from 1 to 4100: match-length codes at both ends of the table
    # (short_and_long was meant for this: its 4-byte words are below the
    # parse's minimum match, so its match lengths stay in one region)
    "zero_repeat_ge_24": ("run_ladder", 4095, 1),
    "zero_repeat_3_23": ("dim", 255, 1),
    "sequences_at_block_ge_64": ("dim", 524288 + 8192 + 5, 1),
    "fcs_1": ("zeros", 1, 1),
    "fcs_2": ("zeros", 256, 1),
    "fcs_4": ("zeros", 65792, 1),
}


def test_device_encoder_census(gpu):
    runs = {}
    for kind, nb, level in set(WITNESS.values()):
        runs.setdefault((nb, level), set()).add(kind)
    seen = {}
    for (nb, level), kinds in sorted(runs.items()):
        names = tuple(k for k in ep.NAMES if k in kinds)
        chunks = np.stack([family(nb)[ep.NAMES.index(k)] for k in names])
        for k, info in zip(names, check_plain_run(gpu, chunks, level, names)):
            seen[(k, nb, level)] = features(info)
    for feat, wit in WITNESS.items():
        assert feat in seen[wit], (feat, wit, sorted(seen[wit]))
    assert set(WITNESS) >= EMITTED
    # two different accuracy logs among the fitted tables of the witnesses
    logs = {int(x) for feats in seen.values() for f in feats if f.startswith("logs_")
            for x in f.split("_")[1:]}
    assert len(logs) >= 2, logs
    for wit, feats in seen.items():
        assert not unexpected(feats), (wit, unexpected(feats))


# ---- the match-distance ceiling --------------------------------------------------------
OFF_MAX = (1 << 24) - 4     # kZOffMax


@pytest.mark.parametrize("dist", [OFF_MAX, OFF_MAX + 1, (1 << 24) + 4096])
def test_match_distance_ceiling(gpu, monkeypatch, dist):
    """One 18 MiB chunk: 64 KiB of random bytes, zeros, and the same 64 KiB again
    `dist` bytes on, at level 3 with one far range (the tail sees the head).  At
    the largest distance the encoder codes (Offset_Value = distance + 3 < 2^24)
    the blocks inside the copy are matches; one byte further they are not."""
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    T, hw, span = 9, 1024, 65536
    rng = np.random.default_rng(6)
    chunk = np.zeros(T * hw * hw * 2, np.uint8)
    chunk[:span] = rng.integers(0, 256, span, dtype=np.uint8)
    chunk[dist:dist + span] = chunk[:span]
    dims = [(TIME, 0, T, 1), (SPACE, hw, hw, 1), (SPACE, hw, hw, 1)]
    st = gpu.Stage(dims, U16, MEAN, multiscale=False, layer_slots=2, max_batch_frames=T,
                   zstd_flags=gpu.ZSTD_FAR_ONE_RANGE)
    st.append(chunk.view(np.uint16).reshape(T, hw, hw))
    layer, _ = st.copy_layer(0, 0)
    assert st.layout(0)["bytes_per_chunk"] == chunk.size and np.array_equal(layer, chunk)
    st.compress_layer(0, 0, codec=gpu.CODEC_ZSTD, clevel=3, shuffle=0)
    data, _ = st.copy_compressed(0, 0)
    (_, _, _, o, nb), = st.compressed_entries(0, 0)
    assert st.zstd_far_ranges(0) == 1
    st.close()
    fr = data[o:o + nb].tobytes()
    assert zstd_decode(fr, chunk.size) == chunk.tobytes()
    info = inspect(fr)
    assert info["fcs"] == chunk.size and not unexpected(features(info))
    # the blocks that lie inside the copy: random bytes, raw unless matched
    inside = info["blocks"][-(-dist // KBLOCK):(dist + span) // KBLOCK]
    assert len(inside) == 7
    kinds = [(b["type"], b.get("nseq")) for b in inside]
    print(f"distance {dist}: blocks inside the copy {kinds}")
    if dist <= OFF_MAX:
        assert all(t == "compressed" and n > 0 for t, n in kinds), kinds
    else:
        assert all(t == "raw" for t, _ in kinds), kinds


# ---- blosc-LZ4 with the same family ----------------------------------------------------
@pytest.mark.parametrize("shuffle", [0, 1, 2])
@pytest.mark.parametrize("ts", [1, 2])
def test_blosc_lz4_family(gpu, ts, shuffle):
    for nb in (13, 4097, 16384 + 12000, 70001):
        chunks = np.array(family(nb, ep.LZ4_NAMES))
        frames, total, _ = compress_device(gpu, chunks, ts, 5, shuffle)
        assert total == sum(len(f) for f in frames)
        check_frames(frames, chunks, ts, shuffle, 5)
        lz4_round_trip(gpu, chunks, ts, 5, shuffle, pad=5)   # and the device decoder
