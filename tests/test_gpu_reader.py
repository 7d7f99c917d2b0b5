"""GPU tests of the device reader (aqz_reader_*): a level's chunk layer -- raw,
resident in a stage, compressed with any of the three codecs, or gathered from
shard bytes -- comes back as the row-major frames that were appended, bit for
bit (a byte mover: no tolerance), in acquisition order and orientation.  The
expected layers come from the oracle (OracleDims.write_frame_to_chunks,
helpers.expected_stage_layers' twin oracle_cascade for the pyramid levels); the
expected frames are the inputs themselves.  Destinations are painted and
guarded: only bytes [0, frame_bytes) of each destination frame may change."""
import os

import numpy as np
import pytest

from codec_helpers import camera_like
from decoder_helpers import CORRUPT, OK, SKIPPED, load_golden, named_mutations
from helpers import oracle_cascade
from oracle_bindings import (CHANNEL, MEAN, SPACE, TIME, U8, U16, U32, U64,
                             OracleDims, synthetic_frames)

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
BY_SIZE = {1: U8, 2: U16, 4: U32, 8: U64}

GEOMETRIES = {
    # the 16-byte path; a non-identity shard order
    "aligned": [(TIME, 0, 2, 1), (SPACE, 64, 32, 1), (SPACE, 64, 32, 2)],
    # ragged tiles in y and x
    "ragged": [(TIME, 0, 3, 1), (SPACE, 45, 16, 2), (SPACE, 70, 32, 1)],
    # unaligned chunk rows
    "odd": [(TIME, 0, 2, 1), (SPACE, 17, 17, 1), (SPACE, 33, 33, 1)],
    # tile_group_offset and chunk_internal_offset both vary inside a layer; ragged c and z
    "5d": [(TIME, 0, 2, 1), (CHANNEL, 3, 2, 1), (SPACE, 5, 2, 2), (SPACE, 20, 8, 1),
           (SPACE, 24, 16, 1)],
    # tiles taller than one 64-row slab of the kernel's walk, the last slab cut twice
    "tall": [(TIME, 0, 1, 1), (SPACE, 150, 100, 1), (SPACE, 40, 24, 1)],
}


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def read_back(rd, first, count, base=3, pad=24):
    """Frames [first, first + count) into a FILL-painted buffer at an odd base
    with a stride of frame bytes + pad and a guard region behind it; every byte
    outside the frames must keep the fill."""
    torch = _torch()
    fb = rd.layout()["frame_bytes"]
    stride = fb + pad
    buf = torch.full((base + count * stride + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rd.read_frames_ptr(first, count, buf.data_ptr() + base, stride, _stream())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    body = b[base:base + count * stride].reshape(count, stride)
    assert (b[:base] == FILL).all(), "bytes in front of the first frame changed"
    assert (body[:, fb:] == FILL).all(), "bytes between frames changed"
    assert (b[base + count * stride:] == FILL).all(), "guard bytes changed"
    return body[:, :fb]


def as_bytes(frames):
    return np.ascontiguousarray(frames).view(np.uint8).reshape(len(frames), -1)


def oracle_layer(dims, dtype, frames, layer):
    od = OracleDims(dims, dtype)
    F = od.frames_per_chunk_layer()
    buf, has = od.new_layer()
    for f in range(F):
        od.write_frame_to_chunks(layer * F + f, frames[f], buf, has)
    return buf, has


# ---- 1. the un-split kernel alone ----------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_unsplit_raw_layer(gpu, geometry, ts):
    torch = _torch()
    dims, dtype = GEOMETRIES[geometry], BY_SIZE[ts]
    od = OracleDims(dims, dtype)
    F, bpc = od.frames_per_chunk_layer(), od.bytes_per_chunk()
    H, W = dims[-2][1], dims[-1][1]
    frames = synthetic_frames(dtype, F, H, W, 100 + ts)
    buf, has = oracle_layer(dims, dtype, frames, layer=1)   # the tables are periodic in F
    assert has.all()
    want = as_bytes(frames)
    rd = gpu.Reader(dims, dtype)
    lay = rd.layout()
    assert (lay["frame_bytes"], lay["frames_per_layer"], lay["bytes_per_chunk"]) == \
        (H * W * ts, F, bpc)
    assert (lay["width"], lay["height"], lay["chunks_per_layer"]) == \
        (W, H, od.number_of_chunks_in_memory())
    # chunks packed at bytes_per_chunk, then at a pitch with an odd pad (unaligned chunks)
    for pad in (0, 16, 7):
        n = len(has)
        pitched = np.full((n, bpc + pad), 0x5A, dtype=np.uint8)
        pitched[:, :bpc] = buf.reshape(n, bpc)
        dev = torch.from_numpy(pitched).to("cuda")
        rd.load_chunks(dev.data_ptr(), bpc + pad, None, 0, _stream())
        assert np.array_equal(read_back(rd, 0, F), want), (geometry, ts, pad)
        st, bad = rd.status()
        assert bad == 0 and (st == OK).all()
        # an aligned destination: the widest unit the geometry allows
        assert np.array_equal(read_back(rd, 0, F, base=0, pad=32), want), (geometry, ts, pad)
    # sub-ranges, and what is refused
    for first, count in {(min(1, F - 1), 1), (F - 1, 1)}:
        assert np.array_equal(read_back(rd, first, count), want[first:first + count])
    dst = torch.full((2 * lay["frame_bytes"],), FILL, dtype=torch.uint8, device="cuda")
    for first, count, stride in ((F, 1, lay["frame_bytes"]), (F - 1, 2, lay["frame_bytes"]),
                                 (0, F + 1, lay["frame_bytes"]), (0, 1, lay["frame_bytes"] - 1)):
        with pytest.raises(gpu.AqzError) as e:
            rd.read_frames_ptr(first, count, dst.data_ptr(), stride, _stream())
        assert e.value.status == 1
        assert gpu.lib().aqz_last_error()
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    with pytest.raises(gpu.AqzError) as e:
        rd.load_chunks(dev.data_ptr(), bpc - 1, None, 0, _stream())
    assert e.value.status == 1
    rd.close()


def test_read_before_load_is_refused(gpu):
    rd = gpu.Reader(GEOMETRIES["aligned"], U16)
    dst = _torch().empty(rd.layout()["frame_bytes"], dtype=_torch().uint8, device="cuda")
    with pytest.raises(gpu.AqzError) as e:
        rd.read_frames_ptr(0, 1, dst.data_ptr(), dst.numel(), _stream())
    assert e.value.status == 1
    rd.close()


# ---- 2. storage orders, fed from a stage's resident layers -----------------------------
def read_stage_layers(gpu, st, rd, level, n_layers):
    lay = st.layout(level)
    out = []
    for layer in range(n_layers):
        chunks, flags, tag = st.device_layer(level, layer)
        rd.load_chunks(chunks, lay["chunk_pitch"], flags, tag, _stream())
        out.append(read_back(rd, 0, lay["frames_per_layer"]))
    return np.concatenate(out)


def test_storage_order_frame_permutation(gpu):
    acq = GEOMETRIES["5d"]
    perm = [0, 2, 1, 3, 4]
    F = 2 * 3 * 5
    frames = synthetic_frames(U16, 2 * F, 20, 24, 7)
    st = gpu.Stage(acq, U16, MEAN, multiscale=False, storage_order=perm, layer_slots=4,
                   max_batch_frames=16)
    st.append(frames)
    st.synchronize()
    rd = gpu.Reader(acq, U16, storage_order=perm)
    assert rd.layout()["frames_per_layer"] == F == st.layout(0)["frames_per_layer"]
    got = read_stage_layers(gpu, st, rd, 0, 2)
    assert np.array_equal(got, as_bytes(frames))
    rd.close()
    st.close()


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", [(64, 64, 32, 32), (45, 70, 16, 32)])
def test_storage_order_xy_swap(gpu, shape, ts):
    """y and x swapped in storage: the stage stores transposed frames, the reader
    hands the acquired orientation back.  45 x 70 cuts the LDS transpose tiles at
    both edges."""
    H, W, th, tw = shape
    dtype = BY_SIZE[ts]
    acq = [(TIME, 0, 2, 1), (CHANNEL, 2, 1, 1), (SPACE, H, th, 1), (SPACE, W, tw, 1)]
    frames = synthetic_frames(dtype, 8, H, W, 31 + ts)
    st = gpu.Stage(acq, dtype, MEAN, storage_order=[0, 1, 3, 2], layer_slots=4,
                   max_batch_frames=4)
    st.append(frames)
    st.synchronize()
    rd = gpu.Reader(acq, dtype, storage_order=[0, 1, 3, 2])
    lay = rd.layout()
    assert (lay["width"], lay["height"], lay["frames_per_layer"]) == (W, H, 4)
    got = read_stage_layers(gpu, st, rd, 0, 2)
    assert np.array_equal(got, as_bytes(frames))
    rd.close()
    st.close()


# ---- 3. through the codecs -------------------------------------------------------------
PYR = [(TIME, 0, 4, 2), (SPACE, 96, 32, 2), (SPACE, 80, 32, 2)]
_pyr = {}


def pyramid_inputs():
    """Frames and, per level, the images the oracle's cascade emits for them."""
    if not _pyr:
        rng = np.random.default_rng(11)
        frames = camera_like(rng, 8 * 96 * 80, np.uint16).reshape(8, 96, 80)
        _, per_frame = oracle_cascade(PYR, U16, MEAN, frames)
        levels = {0: list(frames)}
        for got in per_frame:
            for l, img in got.items():
                levels.setdefault(l, []).append(img)
        _pyr.update(frames=frames, levels=levels)
    return _pyr["frames"], _pyr["levels"]


@pytest.mark.parametrize("codec,shuffle,mem", [
    ("lz4", 1, "device"), ("lz4", 2, "device"), ("lz4", 1, "host"), ("lz4", 2, "pinned"),
    ("blosc-zstd", 1, "device"), ("zstd", 0, "device")])
def test_compressed_layers_of_every_level(gpu, codec, shuffle, mem):
    torch = _torch()
    frames, levels = pyramid_inputs()
    code = {"lz4": gpu.CODEC_BLOSC_LZ4, "blosc-zstd": gpu.CODEC_BLOSC_ZSTD,
            "zstd": gpu.CODEC_ZSTD}[codec]
    family = gpu.DECODE_CODEC_LZ4 if codec == "lz4" else gpu.DECODE_CODEC_ZSTD
    zstd_on_host = codec != "lz4" and os.environ.get("AQZ_ZSTD_HOST") == "1"
    st = gpu.Stage(PYR, U16, MEAN, layer_slots=2, max_batch_frames=4)
    L = st.n_levels()
    assert L >= 2 and set(levels) == set(range(L))
    try:
        readers = [gpu.Reader(st.level_dims(l), U16, codecs=family) for l in range(L)]
    except gpu.AqzError as e:
        if e.status == 4:
            pytest.skip("device zstd decode not implemented")
        raise
    got = {l: [] for l in range(L)}
    seen = set()
    for b in range(0, len(frames), 4):
        st.append(np.ascontiguousarray(frames[b:b + 4]))
        for l in range(L):
            layer = st.frames_written(l) // st.layout(l)["frames_per_layer"] - 1
            if layer < 0 or (l, layer) in seen:
                continue
            seen.add((l, layer))
            try:
                st.compress_layer(l, layer, codec=code, clevel=3, shuffle=shuffle)
            except gpu.AqzError as e:
                if e.status == 4:
                    pytest.skip("device zstd path not implemented")
                raise
            off = st.compressed_offsets(l, layer)
            total = int(off[-1])
            if zstd_on_host:
                data, _ = st.copy_compressed(l, layer)
                dev = torch.from_numpy(np.ascontiguousarray(data)).to("cuda")
            else:
                dev = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
                st.copy_compressed_async(l, layer, dev.data_ptr(), total)   # device to device
                st.wait_copies()
            if mem == "device":
                src = dev
            elif mem == "host":
                src = dev.cpu().numpy()
            else:
                src = gpu.HostBuffer(max(total, 1))
                src.array[:total] = dev.cpu().numpy()[:total]
            rd = readers[l]
            rd.load_frames(src, off, None, code, frames_bytes=total, stream_ptr=_stream())
            got[l].append(read_back(rd, 0, rd.layout()["frames_per_layer"]))
            status, bad = rd.status()
            assert bad == 0 and (status == OK).all(), (l, layer, status)
    for l in range(L):
        assert len(got[l]) >= 2, "at least two layers per level"
        want = as_bytes(np.stack(levels[l]))
        assert np.array_equal(np.concatenate(got[l]), want), (codec, shuffle, mem, l)
    for rd in readers:
        rd.close()
    st.close()


def test_load_frames_argument_errors(gpu):
    dims = GEOMETRIES["aligned"]
    rd = gpu.Reader(dims, U16, codecs=gpu.DECODE_CODEC_LZ4)
    n, bpc = rd.layout()["chunks_per_layer"], rd.layout()["bytes_per_chunk"]
    blob = np.zeros(n * bpc, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * bpc
    order = np.arange(n, dtype=np.uint32)

    def refused(*a, **k):
        with pytest.raises(gpu.AqzError) as e:
            rd.load_frames(*a, **k)
        assert e.value.status == 1
        assert gpu.lib().aqz_last_error()

    bad = order.copy()
    bad[1] = n
    refused(blob, off, bad, gpu.CODEC_NONE)                       # entry outside the layer
    bad[1] = 0
    refused(blob, off, bad, gpu.CODEC_NONE)                       # listed twice
    dec = off.copy()
    dec[2] = dec[1] - 1
    refused(blob, dec, order, gpu.CODEC_NONE)                     # not monotonic
    refused(blob, off, order, gpu.CODEC_NONE, frames_bytes=int(off[-1]) - 1)
    refused(blob, off, order, gpu.CODEC_ZSTD)                     # not created for it
    refused(blob, off, order, gpu.CODEC_BLOSC_ZSTD)
    refused(blob, off, order, 7)
    refused(blob, off[:-1], None, gpu.CODEC_NONE)                 # NULL order: every chunk
    # and the same arrays are accepted as stored chunks
    rd.load_frames(blob, off, order, gpu.CODEC_NONE)
    assert not read_back(rd, 0, 2).any()
    # a stored frame that is not bytes_per_chunk long
    off2 = off.copy()
    off2[-1] -= 1
    rd.load_frames(blob, off2, order, gpu.CODEC_NONE, frames_bytes=int(off2[-1]))
    st, nbad = rd.status()
    assert nbad == 1 and st[n - 1] == gpu.DECODE_BAD_HEADER and (st[:n - 1] == OK).all()
    rd.close()


# ---- 4. unwritten chunks, 5. shard bytes -------------------------------------------------
HOLE = [(TIME, 0, 2, 2), (SPACE, 64, 32, 2), (SPACE, 96, 32, 2)]
HOLE_CHUNK = 1 * 3 + 1          # tile (1, 1) of the 2 x 3 tiles


def hole_stage(gpu, n_frames=4):
    rng = np.random.default_rng(3)
    frames = camera_like(rng, n_frames * 64 * 96, np.uint16).reshape(n_frames, 64, 96)
    frames[:, 32:64, 32:64] = 0
    st = gpu.Stage(HOLE, U16, MEAN, multiscale=False, layer_slots=2, max_batch_frames=4)
    st.append(frames)
    st.synchronize()
    return st, frames


def test_unwritten_chunks_read_as_zeros(gpu):
    st, frames = hole_stage(gpu)
    want = as_bytes(frames)
    exp_buf, exp_has = oracle_layer(HOLE, U16, frames[:2], 0)
    assert exp_has[HOLE_CHUNK] == 0 and exp_has.sum() == len(exp_has) - 1
    rd = gpu.Reader(HOLE, U16, codecs=gpu.DECODE_CODEC_LZ4)
    n = rd.layout()["chunks_per_layer"]
    # the stage's own has-data words
    chunks, flags, tag = st.device_layer(0, 0)
    rd.load_chunks(chunks, st.layout(0)["chunk_pitch"], flags, tag, _stream())
    assert np.array_equal(read_back(rd, 0, 2), want[:2])
    status, bad = rd.status()
    assert bad == 0 and status[HOLE_CHUNK] == SKIPPED and (np.delete(status, HOLE_CHUNK) == OK).all()
    # the zero-length frame the stage emits for it
    st.compress_layer(0, 0, codec=gpu.CODEC_BLOSC_LZ4, clevel=5, shuffle=1)
    data, off = st.copy_compressed(0, 0)
    entries = st.compressed_entries(0, 0)
    assert [nb for c, _, _, _, nb in entries if c == HOLE_CHUNK] == [0]
    rd.load_frames(data, off, None, gpu.CODEC_BLOSC_LZ4, stream_ptr=_stream())
    assert np.array_equal(read_back(rd, 0, 2), want[:2])
    status, bad = rd.status()
    assert bad == 0 and status[HOLE_CHUNK] == SKIPPED and (np.delete(status, HOLE_CHUNK) == OK).all()
    # a list that omits chunks: the hole, and chunk 0, whose pixels then read as zeros too
    keep = [(c, o, nb) for c, _, _, o, nb in entries if c not in (HOLE_CHUNK, 0)]
    blob = b"".join(bytes(data[o:o + nb]) for _, o, nb in keep)
    offs = np.cumsum([0] + [nb for _, _, nb in keep]).astype(np.uint64)
    rd.load_frames(np.frombuffer(blob, dtype=np.uint8).copy(), offs, [c for c, _, _ in keep],
                   gpu.CODEC_BLOSC_LZ4, stream_ptr=_stream())
    zeroed = frames[:2].copy()
    zeroed[:, 0:32, 0:32] = 0
    assert np.array_equal(read_back(rd, 0, 2), as_bytes(zeroed))
    status, bad = rd.status()
    assert bad == 0 and status[0] == SKIPPED and status[HOLE_CHUNK] == SKIPPED
    assert (np.delete(status, [0, HOLE_CHUNK]) == OK).all() and len(status) == n
    rd.close()
    st.close()


def test_frames_gathered_from_shard_bytes(gpu):
    st, frames = hole_stage(gpu)
    cps, n_shards, lps = st.shard_geometry(0)
    assert lps == 2
    asm = gpu.ShardAssembler(st, 0)
    where = {}
    for layer in range(2):
        st.compress_layer(0, layer, codec=gpu.CODEC_BLOSC_LZ4, clevel=5, shuffle=2)
        data, _ = st.copy_compressed(0, layer)
        entries = st.compressed_entries(0, layer)
        asm.add_layer(data, entries)
        where[layer] = {c: (shard, internal) for c, shard, internal, _, _ in entries}
    blobs = asm.finalize()
    tables = []
    for blob in blobs:
        off, ext, ok = gpu.shard_table_parse(blob[-(16 * cps + 4):], cps)
        assert ok
        tables.append((off, ext))
    rd = gpu.Reader(HOLE, U16, codecs=gpu.DECODE_CODEC_LZ4)
    n = rd.layout()["chunks_per_layer"]
    unwritten = (1 << 64) - 1
    for layer in range(2):
        parts, chunks = [], []
        for c in range(n):
            shard, internal = where[layer][c]
            off, ext = int(tables[shard][0][internal]), int(tables[shard][1][internal])
            if c == HOLE_CHUNK:
                assert off == ext == unwritten
                continue
            parts.append(blobs[shard][off:off + ext])
            chunks.append(c)
        blob = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
        offs = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
        rd.load_frames(blob, offs, chunks, gpu.CODEC_BLOSC_LZ4, stream_ptr=_stream())
        assert np.array_equal(read_back(rd, 0, 2), as_bytes(frames[2 * layer:2 * layer + 2]))
        status, bad = rd.status()
        assert bad == 0 and status[HOLE_CHUNK] == SKIPPED
    rd.close()
    st.close()


def test_second_load_waits_for_reads_on_another_stream(gpu):
    """Loads on one stream, reads on another, the second load enqueued while the
    reads of the first layer are still queued: both layers come back exact (the
    reader orders a load behind the reads of the previous layer and a read behind
    its load, whichever streams they are on)."""
    torch = _torch()
    dims = [(TIME, 0, 8, 1), (SPACE, 1024, 256, 1), (SPACE, 1024, 256, 1)]
    rng = np.random.default_rng(21)
    frames = camera_like(rng, 16 * 1024 * 1024, np.uint16).reshape(16, 1024, 1024)
    st = gpu.Stage(dims, U16, MEAN, multiscale=False, layer_slots=2, max_batch_frames=16)
    st.append(frames)
    st.synchronize()
    layers = []
    for layer in range(2):
        st.compress_layer(0, layer, codec=gpu.CODEC_BLOSC_LZ4, clevel=5, shuffle=1)
        off = st.compressed_offsets(0, layer)
        dev = torch.empty(int(off[-1]), dtype=torch.uint8, device="cuda")
        st.copy_compressed_async(0, layer, dev.data_ptr(), dev.numel())
        st.wait_copies()
        layers.append((dev, off))
    rd = gpu.Reader(dims, U16, codecs=gpu.DECODE_CODEC_LZ4)
    fb = rd.layout()["frame_bytes"]
    out = [torch.full((8 * fb,), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    loads, reads = torch.cuda.Stream(), torch.cuda.Stream()
    for (dev, off), dst in zip(layers, out):
        rd.load_frames(dev, off, None, gpu.CODEC_BLOSC_LZ4, stream_ptr=loads.cuda_stream)
        for f in range(8):
            rd.read_frames_ptr(f, 1, dst.data_ptr() + f * fb, fb, reads.cuda_stream)
    torch.cuda.synchronize()
    assert rd.status()[1] == 0
    want = as_bytes(frames)
    for layer in range(2):
        got = out[layer].cpu().numpy().reshape(8, fb)
        assert np.array_equal(got, want[8 * layer:8 * layer + 8]), layer
    rd.close()
    st.close()


# ---- 6. damage -------------------------------------------------------------------------
def test_damaged_frame_is_a_status_and_spares_its_neighbours(gpu):
    """One frame of the layer is a c-blosc golden frame with a named mutation whose
    status is CORRUPT (the host parse of the same bytes runs under ASan in
    tests/test_decoder_cpu.py).  Defined status, every other chunk exact, nothing
    written outside the destination frames."""
    torch = _torch()
    golden = {name: fr for name, fr, *_ in load_golden()}["camera_ts4_sh1"]
    name, damaged, chunk_bytes, want_status = next(
        m for m in named_mutations(golden) if m[0] == "match_offset_0")
    assert want_status == CORRUPT and chunk_bytes == 3000
    # 3 x 5 x 50 u32 pixels = 3000 bytes per chunk; ragged in y
    dims = [(TIME, 0, 3, 1), (SPACE, 12, 5, 1), (SPACE, 100, 50, 1)]
    od = OracleDims(dims, U32)
    assert od.bytes_per_chunk() == chunk_bytes
    n, F = od.number_of_chunks_in_memory(), od.frames_per_chunk_layer()
    rng = np.random.default_rng(8)
    frames = camera_like(rng, F * 12 * 100, np.uint32).reshape(F, 12, 100)
    buf, _ = oracle_layer(dims, U32, frames, 0)
    src = torch.from_numpy(buf).to("cuda")
    comp = gpu.Compressor(chunk_bytes, 4, clevel=5, shuffle=1)
    cap = comp.max_bytes(n)
    fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), chunk_bytes, n, fr.data_ptr(), cap, off.data_ptr(), _stream())
    torch.cuda.synchronize()
    o, data = off.cpu().numpy(), fr.cpu().numpy()
    victim = 3
    parts = [bytes(data[o[c]:o[c + 1]]) for c in range(n)]
    parts[victim] = damaged
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    rd = gpu.Reader(dims, U32, codecs=gpu.DECODE_CODEC_LZ4)
    rd.load_frames(blob, offs, list(range(n)), gpu.CODEC_BLOSC_LZ4, stream_ptr=_stream())
    got = read_back(rd, 0, F)                  # asserts the fill outside the frames
    status, bad = rd.status()
    assert bad == 1 and status[victim] == CORRUPT and (np.delete(status, victim) == OK).all()
    # pixels of the other chunks are exact: mask the victim's tile (ty 1, tx 1) out
    got = got.view(np.uint32).reshape(F, 12, 100).copy()
    want = frames.copy()
    assert victim == 1 * 2 + 1
    got[:, 5:10, 50:100] = 0
    want[:, 5:10, 50:100] = 0
    assert np.array_equal(got, want)
    comp.close()
    rd.close()


# ---- 7. memory ---------------------------------------------------------------------------
def test_reader_memory_is_what_the_estimator_says(gpu):
    torch = _torch()
    dims = [(TIME, 0, 8, 1), (SPACE, 1024, 256, 1), (SPACE, 1024, 256, 1)]
    bpc, n = 8 * 256 * 256 * 2, 16
    codecs = gpu.DECODE_CODEC_LZ4

    def cycle(rd, fr, offs, dst):
        lay = rd.layout()
        rd.load_frames(fr, offs, list(range(lay["chunks_per_layer"])), gpu.CODEC_BLOSC_LZ4,
                       stream_ptr=_stream())
        rd.read_frames_ptr(0, lay["frames_per_layer"], dst.data_ptr(), lay["frame_bytes"],
                           _stream())
        torch.cuda.synchronize()
        assert rd.status()[1] == 0

    def layer_frames(nb, nn, out_bytes):
        """Frames of a compressible layer, made before anything is measured (the
        compressor allocates its scratch in its first run), and a destination."""
        comp = gpu.Compressor(nb, 2, clevel=5, shuffle=1)
        src = torch.zeros(nn * nb, dtype=torch.uint8, device="cuda")
        src[::7] = 3
        fr = torch.empty(comp.max_bytes(nn), dtype=torch.uint8, device="cuda")
        off = torch.empty(nn + 1, dtype=torch.int64, device="cuda")
        comp.run_ptr(src.data_ptr(), nb, nn, fr.data_ptr(), fr.numel(), off.data_ptr(), _stream())
        torch.cuda.synchronize()
        offs = off.cpu().numpy().astype(np.uint64)
        comp.close()
        return fr, offs, torch.empty(out_bytes, dtype=torch.uint8, device="cuda")

    # every kernel involved has run once (code objects are loaded on first use)
    small = GEOMETRIES["aligned"]
    warm = gpu.Reader(small, U16, codecs=codecs)
    wl = warm.layout()
    cycle(warm, *layer_frames(wl["bytes_per_chunk"], wl["chunks_per_layer"],
                              wl["frames_per_layer"] * wl["frame_bytes"]))
    warm.close()
    cycle_args = layer_frames(bpc, n, 8 * 1024 * 1024 * 2)
    torch.cuda.synchronize()
    want = gpu.reader_device_bytes(dims, U16, codecs=codecs)
    assert want > 3 * n * bpc           # layer buffer, staging and decoder scratch
    free0 = torch.cuda.mem_get_info()[0]
    rd = gpu.Reader(dims, U16, codecs=codecs)
    free1 = torch.cuda.mem_get_info()[0]
    assert rd.device_bytes() == want
    # five allocations (tables, layer, staging, two of the decoder), each rounded up to
    # the runtime's 2 MiB granule at the most
    assert abs((free0 - free1) - want) <= 5 * (2 << 20), (free0 - free1, want)
    cycle(rd, *cycle_args)
    cycle(rd, *cycle_args)
    assert torch.cuda.mem_get_info()[0] == free1
    rd.close()
    torch.cuda.synchronize()
    assert abs(torch.cuda.mem_get_info()[0] - free0) <= 5 * (2 << 20)
