"""GPU tests of the per-layer bookkeeping past its first pass: more than 256 chunks
per run or layer, more than 256 streams / segments / blocks inside one chunk, a layer
whose frames add up past 4 GiB, and the chunk-count limit of the block shuffle.

The bookkeeping kernels work in passes of one workgroup (256 chunks, streams or
segments per pass; 64 blocks per wave step) and carry a running sum between passes.
Every expectation here is a reference's: the input bytes themselves, the oracle's
chunk layers, c-blosc / libzstd / the oracle decoding the device's frames, or a value
derived from the format (a memcpyed frame is its chunk plus 16 bytes).

Which test drives the second pass of which loop, and the condition it asserts:
  scan_offsets, carry across passes    test_many_small_chunks (n of 257, 513, 1025;
                                       offsets non-decreasing, offsets[n] = sum of frames)
  scan_offsets, sums of one pass       test_layer_frames_past_4gib (offsets[i] = i * frame)
  scan_offsets, order of 256 and up    test_stage_layers_past_256_chunks (entries
                                       shard-major by the oracle, not the identity)
  chunk_layout, streams of a chunk     test_lz4_chunk_of_more_than_256_streams (301 and
                                       521 streams counted from the frame)
  write_frames, block starts           the same (301 and 261 blocks from the header)
  zstd_chunk, segments of a chunk      test_blosc_zstd_chunk_of_more_than_256_segments (258)
  decoders' frame_ref, slot >= 256     test_many_small_chunks, test_mixed_run_of_600_frames;
                                       with an order: the verify and reader steps of
                                       test_stage_layers_past_256_chunks (n0 > 256)
  verify_layer's reduction             test_stage_layers_past_256_chunks ((2, 255) and
                                       (1, 256): damage either side of the pass)
  parallel zstd tables and counts      test_many_small_chunks[zstd-*] (parallel_frames = n,
                                       blocks and sequences = the sums inspect gives)
  unsplit_chunk_table, has_data tags   the load_chunks steps of the two stage tests
                                       (chunks without data on both sides of 256)
A library whose scan_offsets drops its carry fails the 256- and 257-chunk cases, one
whose chunk_layout / zstd_chunk drop theirs fails the four tests of section 2 (tried
with scratch builds, not kept)."""
import time

import numpy as np
import pytest

from codec_helpers import (camera_like, header, libblosc, libblosc_decode, oracle_decode,
                           zstd_decode)
from decoder_helpers import (BAD_HEADER, CORRUPT, MUTATED, OK, SKIPPED, UNSUPPORTED,
                             streams)
from decoder_helpers import load_golden as load_lz4_golden
from decoder_helpers import named_mutations as lz4_named_mutations
from helpers import expected_stage_layers
from oracle_bindings import MEAN, SPACE, TIME, U8, OracleDims, OracleDownsampler
from test_gpu_codec import parse_shard
from test_gpu_decode import FILL, GUARD, _literal_byte, decode_host_frames, run_decoder
from test_gpu_reader import as_bytes, read_back
from test_gpu_zstddec import host_frames
from zstddec_helpers import blosc_streams, inspect, reference_decode
from zstddec_helpers import load_golden as load_zstd_golden
from zstddec_helpers import named_mutations as zstd_named_mutations

pytestmark = pytest.mark.gpu

UINT32_MAX = (1 << 32) - 1
MAGIC = b"\x28\xb5\x2f\xfd"


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def _codes(gpu):
    return {"lz4": gpu.CODEC_BLOSC_LZ4, "blosc-zstd": gpu.CODEC_BLOSC_ZSTD,
            "zstd": gpu.CODEC_ZSTD}


def host_decode(codec, fr, nbytes):
    """The frame decoded by the host references: the oracle's blosc1-LZ4 decoder,
    libzstd (under the restated blosc container for blosc-zstd), and c-blosc where the
    image has it; they must agree."""
    fr = bytes(fr)
    if codec == "zstd":
        return zstd_decode(fr, nbytes)
    out = oracle_decode(fr) if codec == "lz4" else reference_decode(fr, nbytes)
    if libblosc() is not None:
        assert libblosc_decode(fr) == out
    return out


def compress_painted(gpu, chunks: np.ndarray, ts, codec, clevel, shuffle):
    """The device compressor into a FILL-painted destination of max_bytes + GUARD:
    (frames tensor, capacity, offsets tensor, offsets on the host); everything from
    offsets[n] on must keep the fill."""
    torch = _torch()
    n, nb = chunks.shape
    src = torch.from_numpy(np.array(chunks)).to("cuda")
    comp = gpu.Compressor(nb, ts, codec=codec, clevel=clevel, shuffle=shuffle)
    cap = comp.max_bytes(n)
    fr = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(), _stream())
    torch.cuda.synchronize()
    comp.close()
    o = off.cpu().numpy()
    assert o[0] == 0 and (np.diff(o) >= 0).all() and 0 < o[n] <= cap, o[[0, n]]
    assert bool((fr[int(o[n]):] == FILL).all()), "bytes behind the last frame changed"
    return fr, cap, off, o


# ---- 1. many small chunks -------------------------------------------------------------
COUNTS = (255, 256, 257, 513, 1025)
SIZES = (2048, 330)        # 330: no multiple of 4, frame starts of every alignment
_payload = {}


def many_chunks(n, nb):
    """n chunks of nb bytes cycling through camera-like, zeros, random and ramp, the
    chunk index XOR-ed into the first two bytes; no two chunks are equal."""
    if (n, nb) not in _payload:
        rng = np.random.default_rng(1000 * n + nb)
        out = np.empty((n, nb), dtype=np.uint8)
        for i in range(n):
            k = i % 4
            if k == 0:
                out[i] = camera_like(rng, nb // 2, np.uint16).view(np.uint8)
            elif k == 1:
                out[i] = 0
            elif k == 2:
                out[i] = rng.integers(0, 256, nb, dtype=np.uint8)
            else:
                out[i] = (np.arange(nb) % 251).astype(np.uint8)
            out[i, 0] ^= i & 0xff
            out[i, 1] ^= i >> 8
        assert len({c.tobytes() for c in out}) == n
        out.setflags(write=False)
        _payload[(n, nb)] = out
    return _payload[(n, nb)]


SMALL_CODECS = [("lz4", 5, 0, 1), ("lz4", 5, 1, 1), ("lz4", 5, 2, 1), ("lz4", 5, 0, 2),
                ("lz4", 5, 1, 2), ("lz4", 5, 2, 2), ("lz4", 0, 1, 2),
                ("blosc-zstd", 3, 1, 2), ("blosc-zstd", 5, 2, 2), ("zstd", 1, 0, 2),
                ("zstd", 3, 0, 2)]


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("codec,clevel,shuffle,ts", SMALL_CODECS)
def test_many_small_chunks(gpu, codec, clevel, shuffle, ts, n):
    """scan_offsets past its first pass of 256 chunks (n = 257 and up: the carry; 513,
    1025: three and five passes), and the decoders' frame references and per-chunk
    tables at slots of 256 and above."""
    Z, P = gpu.DECODE_CODEC_ZSTD, gpu.DECODE_ZSTD_PARALLEL
    for nb in SIZES:
        chunks = many_chunks(n, nb)
        what = (codec, clevel, shuffle, ts, n, nb)
        fr, cap, off, o = compress_painted(gpu, chunks, ts, _codes(gpu)[codec], clevel, shuffle)
        frames = host_frames(fr, off)
        assert int(o[n]) == sum(len(f) for f in frames), what
        for i, f in enumerate(frames):
            assert len(f) > 0, (what, i)
            if codec == "zstd":
                assert f[:4] == MAGIC, (what, i)
            else:
                h = header(f)
                assert h["cbytes"] == len(f) and h["nbytes"] == nb and h["typesize"] == ts
                assert (h["flags"] >> 5) == (1 if codec == "lz4" else 4)
                if clevel == 0:
                    assert h["flags"] & 0x2
            assert host_decode(codec, f, nb) == chunks[i].tobytes(), (what, i)
        decoders = [gpu.DECODE_CODEC_LZ4] if codec == "lz4" else [Z, Z | P]
        for codecs in decoders:
            dec = gpu.Decompressor(nb, n, codecs=codecs)
            got = run_decoder(gpu, dec, fr, cap, off, n, nb, pad=5)
            counts = dec.last_run_counts()
            dec.close()
            assert (got.status == OK).all(), (what, codecs, np.flatnonzero(got.status != OK))
            bad = np.flatnonzero((got.chunks != chunks).any(axis=1))
            assert bad.size == 0, (what, codecs, bad[:8])
            assert got.pads_untouched, (what, codecs)
            if codecs == Z | P and codec == "zstd":
                assert counts["parallel_frames"] == n and counts["serial_frames"] == 0, \
                    (what, counts)
                info = [inspect(f) for f in frames]
                assert counts["blocks"] == sum(1 for i in info for b in i["blocks"]
                                               if b["type"] == "compressed"), (what, counts)
                assert counts["sequences"] == sum(b.get("nseq", 0) for i in info
                                                  for b in i["blocks"]), (what, counts)
            elif codecs == Z | P:
                assert counts["parallel_frames"] == 0, (what, counts)   # blosc frames: serial


@pytest.mark.parametrize("decoder", ["lz4", "zstd", "zstd-parallel"])
def test_mixed_run_of_600_frames(gpu, decoder):
    """600 frames in one run: good frames at the even positions, zero-length frames at
    the odd ones, and every named mutation of the decoder's family -- the first three at
    255, 256 and 511, either side of the second and third pass.  Each status is the one
    named_mutations states; every good frame decodes exactly."""
    if decoder == "lz4":
        good = {name: fr for name, fr, *_ in load_lz4_golden()}[MUTATED[0]]
        nb = header(good)["nbytes"]
        want = oracle_decode(good)
        muts = [(name, data, st) for name, data, cb, st in lz4_named_mutations(good) if cb == nb]
        codecs = gpu.DECODE_CODEC_LZ4
    else:
        golden, _ = load_zstd_golden()
        good, nb = golden["text_windowed"]
        want = zstd_decode(good, nb)
        muts = [(name, data, st) for name, data, n, st in zstd_named_mutations(golden)
                if n == nb and name.startswith("text_windowed:")]
        codecs = gpu.DECODE_CODEC_ZSTD | (gpu.DECODE_ZSTD_PARALLEL if decoder != "zstd" else 0)
    assert len(muts) >= 8 and {BAD_HEADER, CORRUPT, UNSUPPORTED} <= {st for *_, st in muts}
    total = 600
    run = [good if i % 2 == 0 else b"" for i in range(total)]
    expect = [OK if i % 2 == 0 else SKIPPED for i in range(total)]
    where = [255, 256, 511] + [520 + 7 * k for k in range(len(muts) - 3)]
    assert where[-1] < total
    for pos, (name, data, st) in zip(where, muts):
        run[pos], expect[pos] = data, st
    dec = gpu.Decompressor(nb, total, codecs=codecs)
    got = decode_host_frames(gpu, dec, run, nb, pad=11)
    counts = dec.last_run_counts()
    dec.close()
    assert got.pads_untouched
    names = {pos: name for pos, (name, *_) in zip(where, muts)}
    for i in range(total):
        assert got.status[i] == expect[i], (i, names.get(i), got.status[i], expect[i])
        if expect[i] == OK:
            assert got.chunks[i].tobytes() == want, i
        elif expect[i] == SKIPPED:
            assert not got.chunks[i].any(), i
    if decoder == "zstd-parallel":
        n_good = sum(1 for i in range(total) if expect[i] == OK)
        assert counts["parallel_frames"] >= n_good, counts
        blocks = sum(1 for b in inspect(good)["blocks"] if b["type"] == "compressed")
        assert counts["blocks"] >= n_good * blocks, counts


# ---- 2. many streams, segments or blocks inside one chunk --------------------------------
@pytest.mark.parametrize("ts,shuffle,nblocks", [(1, 0, 300), (2, 1, 260), (2, 2, 260)])
def test_lz4_chunk_of_more_than_256_streams(gpu, ts, shuffle, nblocks):
    """chunk_layout's carry over the streams of one chunk and write_frames' block-start
    loop, both past 256: 300 blocks of one stream (typesize 1), and 260 split blocks =
    520 streams and a leftover block (typesize 2; three passes of chunk_layout)."""
    rng = np.random.default_rng(31 + ts + shuffle)
    nb = 4096 * ts * nblocks + 78
    if ts == 1:     # bytes that repeat without a shuffle
        a = camera_like(rng, nb, np.uint8, level=100.0, noise=0.5, amp=20.0)
    else:
        a = camera_like(rng, nb // 2, np.uint16, noise=3.0).view(np.uint8)
    b = (np.arange(nb) % 251).astype(np.uint8)
    b[rng.integers(0, nb, nb // 40)] ^= 0x55
    chunks = np.stack([a, b])
    fr, cap, off, o = compress_painted(gpu, chunks, ts, gpu.CODEC_BLOSC_LZ4, 5, shuffle)
    frames = host_frames(fr, off)
    for i, f in enumerate(frames):
        h = header(f)
        assert not h["flags"] & 0x2, "a memcpyed frame has no streams"
        assert -(-h["nbytes"] // h["blocksize"]) == nblocks + 1 > 256
        st = streams(f)
        assert len(st) == nblocks * ts + 1 and len(st) > 256 and len(st) % 256
        # records back to back behind the block starts, the last one ends the frame
        pos = 16 + 4 * (nblocks + 1)
        for _, _, p, cs, _ in st:
            assert p == pos
            pos += 4 + cs
        assert pos == len(f) == h["cbytes"]
        assert host_decode("lz4", f, nb) == chunks[i].tobytes(), i
    dec = gpu.Decompressor(nb, 2)
    got = run_decoder(gpu, dec, fr, cap, off, 2, nb, pad=9)
    dec.close()
    assert (got.status == OK).all() and got.pads_untouched
    assert np.array_equal(got.chunks, chunks)


def test_blosc_zstd_chunk_of_more_than_256_segments(gpu):
    """zstd_chunk's carry over the segments (blosc blocks of 256 KiB) of one chunk past
    256: one camera-like chunk of 258 segments, the last one short (64.3 MiB, the
    smallest chunk that qualifies)."""
    rng = np.random.default_rng(41)
    nb = 257 * 256 * 1024 + 1000
    chunk = camera_like(rng, nb // 2, np.uint16).view(np.uint8)[None, :]
    fr, cap, off, o = compress_painted(gpu, chunk, 2, gpu.CODEC_BLOSC_ZSTD, 3, 1)
    f = host_frames(fr, off)[0]
    h = header(f)
    assert not h["flags"] & 0x2 and h["flags"] & 0x10
    nseg = -(-h["nbytes"] // h["blocksize"])
    st = blosc_streams(f)
    assert nseg == len(st) == 258 and nseg > 256 and nseg % 256
    pos = 16 + 4 * nseg
    for _, _, p, cs, _ in st:
        assert p == pos
        pos += 4 + cs
    assert pos == len(f) == h["cbytes"]
    assert host_decode("blosc-zstd", f, nb) == chunk[0].tobytes()
    for codecs in (gpu.DECODE_CODEC_ZSTD, gpu.DECODE_CODEC_ZSTD | gpu.DECODE_ZSTD_PARALLEL):
        dec = gpu.Decompressor(nb, 1, codecs=codecs)
        got = run_decoder(gpu, dec, fr, cap, off, 1, nb, pad=9)
        dec.close()
        assert (got.status == OK).all() and got.pads_untouched, codecs
        assert np.array_equal(got.chunks, chunk), codecs


# ---- 3. a stage whose layers have more than 256 chunks -----------------------------------
# level 0: 17 x 16 = 272 chunks (two passes), and 23 x 23 = 529 (three); U8 tiles of
# 32 x 32 x 2 frames = 2048 bytes; shards of 4 x 4 chunks, ragged at the edges
STAGE_GEOMETRY = {
    "17x16": ([(TIME, 0, 2, 2), (SPACE, 544, 32, 4), (SPACE, 512, 32, 4)],
              # rows of pixels, columns of pixels zeroed: chunks 16..31 and 258, 259
              [(slice(32, 64), slice(None)), (slice(512, 544), slice(64, 128))]),
    "23x23": ([(TIME, 0, 2, 2), (SPACE, 736, 32, 4), (SPACE, 736, 32, 4)],
              # chunks 1, 2; 135, 136 (465, 488 when x is stored before y); 506, 507; 512, 513
              [(slice(0, 32), slice(32, 96)), (slice(160, 192), slice(640, 704)),
               (slice(704, 736), slice(0, 64)), (slice(704, 736), slice(192, 256))]),
}
N_FRAMES = 4
_stage_inputs = {}


def stage_inputs(geometry):
    """(dims, frames, the oracle's chunk layers, the oracle's level dims)"""
    if geometry not in _stage_inputs:
        dims, bands = STAGE_GEOMETRY[geometry]
        H, W = dims[1][1], dims[2][1]
        rng = np.random.default_rng(len(geometry) + H)
        frames = camera_like(rng, N_FRAMES * H * W, np.uint8, level=120.0, noise=6.0,
                             amp=40.0).reshape(N_FRAMES, H, W)
        frames[frames == 0] = 1
        for ys, xs in bands:
            frames[:, ys, xs] = 0
        exp, fw, ldims = expected_stage_layers(dims, U8, MEAN, frames)
        n0 = OracleDims(ldims[0], U8).number_of_chunks_in_memory()
        assert n0 > 256 and n0 % 256, n0
        flags = exp[(0, 0)][1]
        assert not flags[:256].all() and not flags[256:].all(), "no-data chunks on both sides"
        assert flags[:256].any() and flags[256:].any()
        frames.setflags(write=False)
        for buf, fl in exp.values():
            buf.setflags(write=False)
            fl.setflags(write=False)
        _stage_inputs[geometry] = (dims, frames, exp, ldims)
    return _stage_inputs[geometry]


def _damaged(codec, frame, want):
    """A copy of the frame with one payload bit flipped that the host reference rejects or
    decodes to other bytes, and the position of the byte."""
    start = _literal_byte(frame) if codec == "lz4" else len(frame) // 2
    for pos in range(start, len(frame)):
        bad = bytearray(frame)
        bad[pos] ^= 0x10
        try:
            same = host_decode(codec, bytes(bad), len(want)) == want
        except Exception:          # the reference rejects the frame
            same = False
        if not same:
            return pos
    raise AssertionError("no byte of this frame matters to the host decoder")


def _gather_from_shards(gpu, blobs, cps, where, n):
    """(frames blob, offsets, chunk of each frame) of one layer out of shard files, by the
    library's parse of their index tables."""
    tables = []
    for blob in blobs:
        o, e, ok = gpu.shard_table_parse(blob[-(16 * cps + 4):], cps)
        assert ok
        tables.append((o, e))
    parts, chunks = [], []
    for c in range(n):
        shard, internal = where[c]
        o, e = int(tables[shard][0][internal]), int(tables[shard][1][internal])
        if o == gpu.SHARD_UNWRITTEN:
            assert e == gpu.SHARD_UNWRITTEN
            continue
        parts.append(blobs[shard][o:o + e])
        chunks.append(c)
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    return blob, offs, chunks


@pytest.mark.parametrize("geometry", list(STAGE_GEOMETRY))
@pytest.mark.parametrize("codec,clevel,shuffle", [("lz4", 5, 2), ("blosc-zstd", 3, 1),
                                                  ("zstd", 3, 0)])
def test_stage_layers_past_256_chunks(gpu, geometry, codec, clevel, shuffle, monkeypatch):
    """Raw layers, compressed entries, shards, on-device verification and the reader of
    a stage whose level-0 layers have 272 / 529 chunks in a shard-major order that is
    not the chunk order, with chunks without data on both sides of index 256."""
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    torch = _torch()
    Z, P = gpu.DECODE_CODEC_ZSTD, gpu.DECODE_ZSTD_PARALLEL
    code = _codes(gpu)[codec]
    dims, frames, exp, ldims = stage_inputs(geometry)
    ods = OracleDownsampler(dims, U8, MEAN, 0)
    st = gpu.Stage(dims, U8, MEAN, layer_slots=2, max_batch_frames=2)
    L = st.n_levels()
    lay = [st.layout(l) for l in range(L)]
    od = [OracleDims(ods.level_dims(l), U8) for l in range(L)]
    assert lay[0]["chunks_per_layer"] == od[0].number_of_chunks_in_memory() > 256
    family = gpu.DECODE_CODEC_LZ4 if codec == "lz4" else Z
    rd = gpu.Reader(st.level_dims(0), U8, codecs=family)
    rows = {}
    where0 = {}
    done = {l: 0 for l in range(L)}
    verified = False
    for b in range(0, N_FRAMES, 2):
        st.append(np.ascontiguousarray(frames[b:b + 2]))
        for l in range(L):
            while done[l] < st.frames_written(l) // lay[l]["frames_per_layer"]:
                layer = done[l]
                done[l] += 1
                want_buf, want_flags = exp[(l, layer)]
                n, bpc = lay[l]["chunks_per_layer"], lay[l]["bytes_per_chunk"]
                # the raw chunk layer
                buf, flags = st.copy_layer(l, layer)
                assert np.array_equal(flags != 0, want_flags != 0), (l, layer)
                assert np.array_equal(buf, want_buf), (l, layer)
                # compressed: every chunk once, shard-major, contiguous
                st.compress_layer(l, layer, codec=code, clevel=clevel, shuffle=shuffle)
                data, off = st.copy_compressed(l, layer)
                ent = st.compressed_entries(l, layer)
                assert sorted(e[0] for e in ent) == list(range(n)), (l, layer)
                # where the oracle puts chunk c of this layer: shard and index inside it
                at = (layer % st.shard_geometry(l)[2]) * n
                key = [(od[l].shard_index_for_chunk(at + c), od[l].shard_internal_index(at + c))
                       for c, *_ in ent]
                assert key == sorted(key), "entries are not shard-major"
                pos = 0
                for (c, shard, internal, o, nbytes), k in zip(ent, key):
                    assert (shard, internal) == k, (l, layer, c)
                    assert o == pos, (l, layer, c)
                    pos += nbytes
                    if not want_flags[c]:
                        assert nbytes == 0, (l, layer, c)
                        continue
                    chunk = want_buf[c * bpc:(c + 1) * bpc].tobytes()
                    assert host_decode(codec, data[o:o + nbytes], bpc) == chunk, (l, layer, c)
                assert pos == int(off[-1]) == len(data)
                if l == 0:
                    assert [e[0] for e in ent] != list(range(n)), "the order is the identity"
                    where0[layer] = {c: (s, i) for c, s, i, _, _ in ent}
                lps = st.shard_geometry(l)[2]
                if (l, layer // lps) not in rows:
                    rows[(l, layer // lps)] = gpu.ShardAssembler(st, l)
                rows[(l, layer // lps)].add_layer(data, ent)
                if l != 0:
                    continue
                # the reader, from the resident layer and the stage's has-data words
                chunks_ptr, flags_ptr, tag = st.device_layer(0, layer)
                rd.load_chunks(chunks_ptr, lay[0]["chunk_pitch"], flags_ptr, tag, _stream())
                got = read_back(rd, 0, 2)
                status, bad = rd.status()
                assert bad == 0 and np.array_equal(status == SKIPPED, want_flags == 0)
                assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
                # the reader, from the stage's frames on the device
                total = int(off[-1])
                dev = torch.empty(total, dtype=torch.uint8, device="cuda")
                st.copy_compressed_async(0, layer, dev.data_ptr(), total)
                st.wait_copies()
                rd.load_frames(dev, off, None, code, frames_bytes=total, stream_ptr=_stream())
                got = read_back(rd, 0, 2)
                status, bad = rd.status()
                assert bad == 0
                assert np.array_equal(status == SKIPPED, want_flags == 0)
                assert (status[want_flags != 0] == OK).all()
                assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
                if verified:
                    continue
                verified = True
                # on-device verification: clean, two damaged frames, the upper one alone
                real = {c: (o, nbytes) for c, _, _, o, nbytes in ent if nbytes}
                lo = max(c for c in real if c < 256)
                hi = min(c for c in real if c >= 256)
                flips = {}
                for c in (lo, hi):
                    o, nbytes = real[c]
                    chunk = want_buf[c * bpc:(c + 1) * bpc].tobytes()
                    flips[c] = o + _damaged(codec, data[o:o + nbytes].tobytes(), chunk)
                both, upper = data.copy(), data.copy()
                both[flips[lo]] ^= 0x10
                both[flips[hi]] ^= 0x10
                upper[flips[hi]] ^= 0x10
                prepared = [None] if codec == "lz4" else [Z, Z | P]
                for codecs in prepared:
                    if codecs is not None:
                        st.verify_prepare(codecs)
                    assert st.verify_layer(0, layer) == (0, UINT32_MAX), codecs
                    d = torch.from_numpy(data.copy()).to("cuda")
                    assert st.verify_layer(0, layer, d.data_ptr(), d.numel()) == (0, UINT32_MAX)
                    d = torch.from_numpy(both).to("cuda")
                    assert st.verify_layer(0, layer, d.data_ptr(), d.numel()) == (2, lo), codecs
                    d = torch.from_numpy(upper).to("cuda")
                    assert st.verify_layer(0, layer, d.data_ptr(), d.numel()) == (1, hi), codecs
    assert verified and done[0] == 2 and all(done[l] >= 1 for l in range(L))
    # shards: the index parses, every written chunk decodes to the oracle's, the rest
    # carry the sentinel
    checked = 0
    for (l, row), asm in rows.items():
        cim, bpc = od[l].number_of_chunks_in_memory(), od[l].bytes_per_chunk()
        blobs = asm.finalize()
        want = {}
        for cl in range(asm.lps):
            layer = row * asm.lps + cl
            if (l, layer) not in exp or layer >= done[l]:
                continue
            buf, flags = exp[(l, layer)]
            for c in range(cim):
                idx = cl * cim + c
                key = (od[l].shard_index_for_chunk(idx), od[l].shard_internal_index(idx))
                want[key] = buf[c * bpc:(c + 1) * bpc].tobytes() if flags[c] else None
        for s, blob in enumerate(blobs):
            offs, exts = parse_shard(blob, asm.cps)
            for i in range(asm.cps):
                w = want.get((s, i))
                if w is None:
                    assert offs[i] == gpu.SHARD_UNWRITTEN and exts[i] == gpu.SHARD_UNWRITTEN
                    continue
                assert host_decode(codec, blob[offs[i]:offs[i] + exts[i]], bpc) == w, (l, s, i)
                checked += 1
        if l == 0:
            # the reader, from the shard files' bytes
            n = lay[0]["chunks_per_layer"]
            for cl in range(asm.lps):
                layer = row * asm.lps + cl
                blob, offs, chunks = _gather_from_shards(gpu, blobs, asm.cps, where0[layer], n)
                flags = exp[(0, layer)][1]
                assert chunks == [c for c in range(n) if flags[c]]
                rd.load_frames(blob, offs, chunks, code, stream_ptr=_stream())
                got = read_back(rd, 0, 2)
                status, bad = rd.status()
                assert bad == 0 and np.array_equal(status == SKIPPED, flags == 0)
                assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
    assert checked > 2 * 256
    rd.close()
    st.close()


@pytest.mark.parametrize("geometry", list(STAGE_GEOMETRY))
@pytest.mark.parametrize("codec,clevel,shuffle", [("lz4", 5, 2), ("blosc-zstd", 3, 1),
                                                  ("zstd", 3, 0)])
def test_reader_past_256_chunks_xy_swapped(gpu, geometry, codec, clevel, shuffle, monkeypatch):
    """The same frames through a stage that stores x before y: the reader hands the
    acquired orientation back, from the stage's frames and from shard bytes, the zeroed
    bands included (chunks never written read as zeros)."""
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    torch = _torch()
    code = _codes(gpu)[codec]
    dims, frames, _, _ = stage_inputs(geometry)
    order = [0, 2, 1]
    st = gpu.Stage(dims, U8, MEAN, multiscale=False, storage_order=order, layer_slots=2,
                   max_batch_frames=2)
    family = gpu.DECODE_CODEC_LZ4 if codec == "lz4" else gpu.DECODE_CODEC_ZSTD
    rd = gpu.Reader(dims, U8, storage_order=order, codecs=family)
    n = rd.layout()["chunks_per_layer"]
    assert n == st.layout(0)["chunks_per_layer"] > 256 and n % 256
    asm = gpu.ShardAssembler(st, 0)
    assert asm.lps == 2
    where = {}
    for layer in range(2):
        st.append(np.ascontiguousarray(frames[2 * layer:2 * layer + 2]))
        st.compress_layer(0, layer, codec=code, clevel=clevel, shuffle=shuffle)
        off = st.compressed_offsets(0, layer)
        ent = st.compressed_entries(0, layer)
        assert [e[0] for e in ent] != list(range(n))
        skipped = {c for c, _, _, _, nbytes in ent if nbytes == 0}
        assert min(skipped) < 256 <= max(skipped)
        chunks_ptr, flags_ptr, tag = st.device_layer(0, layer)
        rd.load_chunks(chunks_ptr, st.layout(0)["chunk_pitch"], flags_ptr, tag, _stream())
        got = read_back(rd, 0, 2)
        status, bad = rd.status()
        assert bad == 0 and set(np.flatnonzero(status == SKIPPED)) == skipped
        assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
        total = int(off[-1])
        dev = torch.empty(total, dtype=torch.uint8, device="cuda")
        st.copy_compressed_async(0, layer, dev.data_ptr(), total)
        st.wait_copies()
        rd.load_frames(dev, off, None, code, frames_bytes=total, stream_ptr=_stream())
        got = read_back(rd, 0, 2)
        status, bad = rd.status()
        assert bad == 0 and set(np.flatnonzero(status == SKIPPED)) == skipped
        assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
        asm.add_layer(dev.cpu().numpy(), ent)
        where[layer] = ({c: (s, i) for c, s, i, _, _ in ent}, skipped)
    blobs = asm.finalize()
    for layer in range(2):
        blob, offs, chunks = _gather_from_shards(gpu, blobs, asm.cps, where[layer][0], n)
        assert set(range(n)) - set(chunks) == where[layer][1]
        rd.load_frames(blob, offs, chunks, code, stream_ptr=_stream())
        got = read_back(rd, 0, 2)
        assert rd.status()[1] == 0
        assert np.array_equal(got, as_bytes(frames[2 * layer:2 * layer + 2])), layer
    rd.close()
    st.close()


# ---- 4. a layer whose frames pass 4 GiB ---------------------------------------------------
BIG_N = 5
BIG_NB = (1 << 30) + 48
TILE_WORDS = 1 << 18            # 1 MiB of int32
# one constant per chunk, every byte of it different from the others' (so two chunks
# differ in every byte), XOR-ed over a random 1 MiB tile with a per-tile counter
CHUNK_KEYS = (0x00000000, 0x1d2e3f40, 0x3a5c7e80, 0x57a9bdc1, 0x74b8fc02)


def big_source(n, nb):
    """n chunks of nb bytes of incompressible data, filled on the device; and nothing of
    it repeats at a distance an encoder here looks back over."""
    torch = _torch()
    assert nb % 4 == 0 and nb // 4 >= 1024 * TILE_WORDS
    g = torch.Generator(device="cuda")
    g.manual_seed(20240607)
    tile = torch.randint(-(1 << 31), (1 << 31) - 1, (TILE_WORDS,), dtype=torch.int32,
                         device="cuda", generator=g)
    counter = (torch.arange(1024, dtype=torch.int64, device="cuda") * 0x01000193 % (1 << 31)) \
        .to(torch.int32)
    src = torch.empty(n * nb, dtype=torch.uint8, device="cuda")
    words = src.view(torch.int32).view(n, nb // 4)
    for c in range(n):
        key = CHUNK_KEYS[c]
        body = words[c, :1024 * TILE_WORDS].view(1024, TILE_WORDS)
        torch.bitwise_xor(tile[None, :], counter[:, None] ^ key, out=body)
        tail = nb // 4 - 1024 * TILE_WORDS
        words[c, 1024 * TILE_WORDS:] = tile[:tail] ^ (key ^ 0x5a5a5a5a)
    return src


@pytest.mark.parametrize("codec,clevel", [("lz4", 0), ("blosc-zstd", 0), ("lz4", 5), ("zstd", 1)])
def test_layer_frames_past_4gib(gpu, codec, clevel):
    """Five incompressible chunks of 1 GiB + 48 bytes: scan_offsets' sums within one pass
    pass 2^32 (the prefix of the fifth frame, the total), and the fifth chunk begins
    above 4 GiB in the source, the frames and the decoded copy.  Regression test of
    scan_offsets summing a pass in 32 bits (five 1 GiB chunks are the smallest input
    that shows it: the last frame landed on top of the first, reported as success).

    blosc frames of such data are memcpyed: chunk + 16 bytes, offsets i * (nb + 16);
    lz4 clevel 5 reaches that through chunk_layout's rule, clevel 0 by store-only.  A
    plain zstd frame is its 9-byte header and a raw block (3-byte header) per 8 KiB.

    On an MI355X (call times of one process per case): lz4 clevel 0 3.7 s, blosc-zstd
    clevel 0 3.6 s, lz4 clevel 5 3.7 s, zstd level 1 6.5 s, of which the serial zstd
    decoder's walk of the five 1 GiB frames is 2.9 s; 23 to 44 GiB of device memory."""
    try:
        _layer_frames_past_4gib(gpu, codec, clevel)
    finally:
        _torch().cuda.empty_cache()     # tens of GiB: not left in the allocator's cache


def _layer_frames_past_4gib(gpu, codec, clevel):
    torch = _torch()
    n, nb = BIG_N, BIG_NB
    code = _codes(gpu)[codec]
    family = gpu.DECODE_CODEC_LZ4 if codec == "lz4" else gpu.DECODE_CODEC_ZSTD
    cap = gpu.compressor_max_bytes(nb, n)
    pitch = nb + 24
    need = (n * nb + cap + GUARD + n * pitch + GUARD + (1 << 30) +      # buffers, a temporary
            gpu.compressor_scratch_bytes((code, clevel, 0), nb, 1, n) +
            gpu.decompressor_scratch_bytes(nb, n, family) + (2 << 30))   # allocator slack
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"needs {need >> 20} MiB of device memory, {free >> 20} MiB free")
    t0 = time.perf_counter()
    src = big_source(n, nb)
    chunk = [src[c * nb:(c + 1) * nb] for c in range(n)]
    for a in range(n):
        for b in range(a + 1, n):
            assert not bool((chunk[a] == chunk[b]).any()), "chunks differ in every byte"
    fr = torch.full((cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    comp = gpu.Compressor(nb, 1, codec=code, clevel=clevel, shuffle=0)
    comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(), _stream())
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    comp.close()
    flen = nb + 16 if codec != "zstd" else 9 + 3 * -(-nb // 8192) + nb
    o = [int(v) for v in off.cpu().numpy()]
    assert o == [i * flen for i in range(n + 1)], o
    assert o[n - 1] > 1 << 32 and (n - 1) * nb > 1 << 32 and o[n] <= cap
    assert bool((fr[o[n]:] == FILL).all()), "bytes behind the last frame changed"
    for c in range(n):
        if codec == "zstd":
            assert bytes(fr[o[c]:o[c] + 4].cpu().numpy()) == MAGIC, c
            continue
        h = header(bytes(fr[o[c]:o[c] + 16].cpu().numpy()))
        assert (h["nbytes"], h["cbytes"], h["flags"] & 0x2) == (nb, nb + 16, 0x2), (c, h)
        assert (h["flags"] >> 5) == (1 if codec == "lz4" else 4) and h["typesize"] == 1
        assert torch.equal(fr[o[c] + 16:o[c] + 16 + nb], chunk[c]), c
    dst = torch.full((n * pitch + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x7f, dtype=torch.int32, device="cuda")
    dec = gpu.Decompressor(nb, n, codecs=family)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    dec.run_ptr(fr.data_ptr(), cap, off.data_ptr(), n, dst.data_ptr(), pitch, nb,
                status.data_ptr(), _stream())
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    dec.close()
    assert status.cpu().tolist() == [OK] * n
    body = dst[:n * pitch].view(n, pitch)
    for c in range(n):
        assert torch.equal(body[c, :nb], chunk[c]), c
    assert bool((body[:, nb:] == FILL).all()) and bool((dst[n * pitch:] == FILL).all())
    print(f"\n{codec} clevel {clevel}: fill + compress {t1 - t0:.2f} s, decode {t3 - t2:.2f} s, "
          f"need {need >> 20} MiB")


# ---- 5. the chunk-count limit -------------------------------------------------------------
def _tiny_chunks(n):
    """n chunks of 32 u16 elements: element k of chunk c is c + (k & 1), so every chunk
    differs and the bit planes of a chunk are short runs."""
    c = np.arange(n, dtype=np.uint32)[:, None]
    k = np.arange(32, dtype=np.uint32)[None, :]
    return ((c + (k & 1)) & 0xffff).astype(np.uint16).view(np.uint8).reshape(n, 64)


def _device_round_trip(gpu, chunks, code, family, clevel, shuffle):
    torch = _torch()
    n, nb = chunks.shape
    fr, cap, off, o = compress_painted(gpu, chunks, 2, code, clevel, shuffle)
    dst = torch.full((n * nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x7f, dtype=torch.int32, device="cuda")
    dec = gpu.Decompressor(nb, n, codecs=family)
    dec.run_ptr(fr.data_ptr(), cap, off.data_ptr(), n, dst.data_ptr(), nb, nb,
                status.data_ptr(), _stream())
    torch.cuda.synchronize()
    dec.close()
    assert bool((status == OK).all())
    assert np.array_equal(dst[:n * nb].cpu().numpy().reshape(n, nb), chunks)
    assert bool((dst[n * nb:] == FILL).all())
    return fr.cpu().numpy(), o


def test_chunk_count_limit_of_the_block_shuffle(gpu):
    """blosc-zstd with a shuffle runs the block shuffle with the chunk index as the
    grid's y dimension: 65535 chunks compress and decode, 65536 are refused with
    AQZ_STATUS_INVALID_ARGUMENT before anything is enqueued (include/aqz_gpu.h,
    aqz_compressor_run).  Codecs without that kernel take 65536 chunks."""
    chunks = _tiny_chunks(65536)
    assert len(np.unique(chunks.view(np.uint64).reshape(65536, 8), axis=0)) == 65536
    f, o = _device_round_trip(gpu, chunks[:65535], gpu.CODEC_BLOSC_ZSTD, gpu.DECODE_CODEC_ZSTD,
                              3, 2)
    for c in (0, 255, 256, 65534):
        fr = f[o[c]:o[c + 1]].tobytes()
        assert header(fr)["flags"] >> 5 == 4
        assert host_decode("blosc-zstd", fr, 64) == chunks[c].tobytes(), c
    torch = _torch()
    src = torch.from_numpy(chunks).to("cuda")
    comp = gpu.Compressor(64, 2, codec=gpu.CODEC_BLOSC_ZSTD, clevel=3, shuffle=2)
    cap = comp.max_bytes(65536)
    fr = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
    off = torch.full((65537,), -1, dtype=torch.int64, device="cuda")
    with pytest.raises(gpu.AqzError) as e:
        comp.run_ptr(src.data_ptr(), 64, 65536, fr.data_ptr(), cap, off.data_ptr(), _stream())
    assert e.value.status == 1
    torch.cuda.synchronize()
    comp.close()
    assert bool((fr == FILL).all()) and bool((off == -1).all()), "a refused run wrote"
    # no shuffle kernel: blosc-lz4 (its own gather) and plain zstd take 2^16 chunks
    f, o = _device_round_trip(gpu, chunks, gpu.CODEC_BLOSC_LZ4, gpu.DECODE_CODEC_LZ4, 5, 2)
    for c in (0, 65535):
        assert host_decode("lz4", f[o[c]:o[c + 1]], 64) == chunks[c].tobytes(), c
    _device_round_trip(gpu, chunks, gpu.CODEC_ZSTD, gpu.DECODE_CODEC_ZSTD, 1, 0)
