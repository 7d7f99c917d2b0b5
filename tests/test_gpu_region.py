"""GPU tests of region reads (aqz_reader_region_chunks, aqz_reader_load_frames_region,
aqz_reader_read_region): a crop of a few frames of a chunk layer comes back bit for
bit (a byte mover: no tolerance) at any origin, size, stride and alignment, from a
load that touches only the crop's chunks.  The expected pixels are the numpy crop
of the frames that were appended; the expected layers come from the oracle
(OracleDims.write_frame_to_chunks) or from a stage.  Destinations are painted and
guarded as tests/test_gpu_reader.py's are: only the width * bpp bytes of the
crop's rows may change."""
import numpy as np
import pytest

from codec_helpers import camera_like
from decoder_helpers import CORRUPT, OK, SKIPPED, load_golden, named_mutations
from oracle_bindings import MEAN, NP_DTYPES, SPACE, TIME, U8, U16, U32, U64, OracleDims, \
    synthetic_frames
from region_helpers import (GEOMETRIES, PERMUTED, XY_ORDER, XY_SHAPES, frame_ranges,
                            regions_of, xy_dims)

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
NOT_LOADED = 5
BY_SIZE = {1: U8, 2: U16, 4: U32, 8: U64}


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


def read_crop(rd, first, count, region, bpp, packed=False):
    """The crop of frames [first, first + count) into a FILL-painted buffer: at an
    odd base with a row stride of width * bpp + 5 and a frame stride with an odd
    pad, or packed at a 16-aligned base.  Every byte outside the crop's rows,
    guard bytes included, must keep the fill.  -> (count, height, width * bpp)."""
    torch = _torch()
    x0, y0, w, h = region
    rb = w * bpp
    if packed:
        base, rs, fs = 0, rb, h * rb
    else:
        base, rs = 3, rb + 5
        fs = (h - 1) * rs + rb + 7
    buf = torch.full((base + count * fs + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    rd.read_region_ptr(first, count, region, buf.data_ptr() + base, rs, fs, _stream())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    at = (base + np.arange(count)[:, None, None] * fs + np.arange(h)[None, :, None] * rs +
          np.arange(rb)[None, None, :])
    outside = np.ones(len(b), dtype=bool)
    outside[at.ravel()] = False
    assert (b[outside] == FILL).all(), "bytes outside the crop's rows changed"
    return b[at]


def read_frames(rd, first, count):
    torch = _torch()
    fb = rd.layout()["frame_bytes"]
    buf = torch.empty(count * fb, dtype=torch.uint8, device="cuda")
    rd.read_frames_ptr(first, count, buf.data_ptr(), fb, _stream())
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(count, fb)


def crop_bytes(frames, first, count, region):
    x0, y0, w, h = region
    c = np.ascontiguousarray(frames[first:first + count, y0:y0 + h, x0:x0 + w])
    return c.view(np.uint8).reshape(count, h, -1)


def oracle_layer(dims, dtype, frames, layer):
    od = OracleDims(dims, dtype)
    F = od.frames_per_chunk_layer()
    buf, has = od.new_layer()
    for f in range(F):
        od.write_frame_to_chunks(layer * F + f, frames[f], buf, has)
    return buf, has


def check_every_region(rd, frames, dims, bpp, rows_along="y"):
    """Every region x frame range x destination shape against the numpy crop; the
    whole frame against read_frames too."""
    F = rd.layout()["frames_per_layer"]
    regions = regions_of(dims, rows_along)
    assert len(regions) >= 8
    for name, region in regions.items():
        for first, count in frame_ranges(F):
            want = crop_bytes(frames, first, count, region)
            for packed in (False, True):
                got = read_crop(rd, first, count, region, bpp, packed)
                assert np.array_equal(got, want), (name, region, first, count, packed)
            if name == "whole":
                assert np.array_equal(got.reshape(count, -1), read_frames(rd, first, count))
    return regions


# ---- 1. raw layers ---------------------------------------------------------------------
@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_region_of_a_raw_layer(gpu, geometry, ts):
    torch = _torch()
    dims, dtype = GEOMETRIES[geometry], BY_SIZE[ts]
    od = OracleDims(dims, dtype)
    F = od.frames_per_chunk_layer()
    H, W = dims[-2][1], dims[-1][1]
    frames = synthetic_frames(dtype, F, H, W, 200 + ts)
    buf, has = oracle_layer(dims, dtype, frames, layer=1)
    assert has.all()
    dev = torch.from_numpy(buf).to("cuda")
    rd = gpu.Reader(dims, dtype)
    rd.load_chunks(dev.data_ptr(), od.bytes_per_chunk(), None, 0, _stream())
    regions = check_every_region(rd, frames, dims, ts)
    if geometry == "tall":
        # rows 60-70 cross a slab boundary; the 100-row tile's second slab is cut, and
        # the frame's last tile row (50 rows) cuts it again
        assert {"rows-60-70", "cut-last-slab", "last-rows"} <= set(regions)
    if geometry == "taller":
        assert "rows-60-70-of-tile-1" in regions
    st, bad = rd.status()
    assert bad == 0 and (st == OK).all()
    rd.close()


def test_region_over_chunks_with_a_foreign_tag(gpu):
    """Chunks whose has_data word is not the layer's tag read as zeros inside the crop."""
    torch = _torch()
    dims, dtype = GEOMETRIES["ragged"], U16
    od = OracleDims(dims, dtype)
    F, n = od.frames_per_chunk_layer(), od.number_of_chunks_in_memory()
    frames = synthetic_frames(dtype, F, 45, 70, 77) | 1
    buf, _ = oracle_layer(dims, dtype, frames, layer=0)
    dev = torch.from_numpy(buf).to("cuda")
    tag = 9
    flags = np.full(n, tag, dtype=np.uint32)
    foreign = [1 * 3 + 1, 2 * 3 + 2]           # tiles (1, 1) and (2, 2) of the 3 x 3
    flags[foreign] = tag + 1
    dflags = torch.from_numpy(flags.view(np.int32)).to("cuda")
    rd = gpu.Reader(dims, dtype)
    rd.load_chunks(dev.data_ptr(), od.bytes_per_chunk(), dflags.data_ptr(), tag, _stream())
    zeroed = frames.copy()
    zeroed[:, 16:32, 32:64] = 0
    zeroed[:, 32:45, 64:70] = 0
    check_every_region(rd, zeroed, dims, 2)
    st, bad = rd.status()
    assert bad == 0 and (st[foreign] == SKIPPED).all() and (np.delete(st, foreign) == OK).all()
    rd.close()


def stage_layer_reader(gpu, acq, dtype, order, frames, batch):
    st = gpu.Stage(acq, dtype, MEAN, multiscale=False, storage_order=order, layer_slots=4,
                   max_batch_frames=batch)
    st.append(frames)
    st.synchronize()
    rd = gpu.Reader(acq, dtype, storage_order=order)
    return st, rd


def test_region_with_the_frame_permuting_storage_order(gpu):
    acq, perm = PERMUTED
    F = 2 * 3 * 5
    frames = synthetic_frames(U16, 2 * F, 20, 24, 7)
    st, rd = stage_layer_reader(gpu, acq, U16, perm, frames, 16)
    assert rd.layout()["frames_per_layer"] == F
    for layer in range(2):
        chunks, flags, tag = st.device_layer(0, layer)
        rd.load_chunks(chunks, st.layout(0)["chunk_pitch"], flags, tag, _stream())
        check_every_region(rd, frames[layer * F:(layer + 1) * F], acq, 2)
    rd.close()
    st.close()


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", XY_SHAPES)
def test_region_with_the_xy_swapped_storage_order(gpu, shape, ts):
    """y and x swapped in storage: the region is in the acquired orientation, and the
    crop comes back in it.  45 x 70 cuts the LDS transpose tiles at both edges."""
    H, W, th, tw = shape
    dtype, acq = BY_SIZE[ts], xy_dims(shape)
    frames = synthetic_frames(dtype, 8, H, W, 41 + ts)
    st, rd = stage_layer_reader(gpu, acq, dtype, XY_ORDER, frames, 4)
    lay = rd.layout()
    assert (lay["width"], lay["height"], lay["frames_per_layer"]) == (W, H, 4)
    for layer in range(2):
        chunks, flags, tag = st.device_layer(0, layer)
        rd.load_chunks(chunks, st.layout(0)["chunk_pitch"], flags, tag, _stream())
        check_every_region(rd, frames[layer * 4:(layer + 1) * 4], acq, ts, rows_along="x")
    rd.close()
    st.close()


# ---- 2. selective load, 3. the window ---------------------------------------------------
SEL = [(TIME, 0, 2, 2), (SPACE, 64, 32, 2), (SPACE, 96, 32, 2)]   # 2 x 3 tiles, 6 chunks
SEL_REGIONS = {
    "one-tile": ((37, 5, 20, 21), [1]),                # inside tile (0, 1)
    "corner": ((29, 27, 9, 11), [0, 1, 3, 4]),         # the four tiles around (32, 32)
    "last-column": ((64, 0, 32, 64), [2, 5]),
}
_sel = {}


def selective_inputs(gpu):
    """One layer of camera-like frames in a stage, and per codec its frames, offsets
    and entries (compressed once, shared by the tests below and left unchanged)."""
    if not _sel:
        rng = np.random.default_rng(17)
        frames = camera_like(rng, 2 * 64 * 96, np.uint16).reshape(2, 64, 96)
        st = gpu.Stage(SEL, U16, MEAN, multiscale=False, layer_slots=2, max_batch_frames=4)
        st.append(frames)
        st.synchronize()
        layers = {}
        for codec, code, shuffle in (("lz4", gpu.CODEC_BLOSC_LZ4, 1),
                                     ("blosc-zstd", gpu.CODEC_BLOSC_ZSTD, 1),
                                     ("zstd", gpu.CODEC_ZSTD, 0)):
            st.compress_layer(0, 0, codec=code, clevel=3, shuffle=shuffle)
            data, off = st.copy_compressed(0, 0)
            entries = st.compressed_entries(0, 0)
            layers[codec] = (code, np.array(data, dtype=np.uint8), np.array(off, dtype=np.uint64),
                             [(c, o, nb) for c, _, _, o, nb in entries])
        st.close()
        _sel.update(frames=frames, layers=layers)
    return _sel["frames"], _sel["layers"]


def family(gpu, codec):
    return gpu.DECODE_CODEC_LZ4 if codec == "lz4" else gpu.DECODE_CODEC_ZSTD


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("codec", ["lz4", "blosc-zstd", "zstd"])
def test_selective_load_reads_only_the_windows_frames(gpu, codec, mem):
    torch = _torch()
    frames, layers = selective_inputs(gpu)
    code, data, off, entries = layers[codec]
    rd = gpu.Reader(SEL, U16, codecs=family(gpu, codec))
    n = rd.layout()["chunks_per_layer"]
    for name, (region, want_set) in SEL_REGIONS.items():
        for first, count in frame_ranges(2):
            chunks = rd.region_chunks(first, count, region)
            assert list(chunks) == want_set, name
            # the bytes of every frame outside the set are overwritten: they are never read
            spoiled = data.copy()
            for c, o, nb in entries:
                if c not in want_set:
                    spoiled[o:o + nb] = 0xFF
            src = torch.from_numpy(spoiled).to("cuda") if mem == "device" else spoiled
            rd.load_frames_region(src, off, first, count, region, None, code,
                                  stream_ptr=_stream())
            status, bad = rd.status()
            assert bad == 0, (name, status)
            assert (status[want_set] == OK).all(), (name, status)
            assert (np.delete(status, want_set) == NOT_LOADED).all(), (name, status)
            assert len(status) == n
            for packed in (False, True):
                got = read_crop(rd, first, count, region, 2, packed)
                assert np.array_equal(got, crop_bytes(frames, first, count, region)), \
                    (codec, mem, name, first, count, packed)
    rd.close()


def test_selective_load_fits_a_reader_the_layer_does_not(gpu):
    frames, layers = selective_inputs(gpu)
    code, data, off, entries = layers["lz4"]
    region, want_set = SEL_REGIONS["corner"]
    needed = sum(nb for c, _, nb in entries if c in want_set)
    assert 0 < needed < int(off[-1])
    rd = gpu.Reader(SEL, U16, codecs=gpu.DECODE_CODEC_LZ4, max_frames_bytes=needed)
    with pytest.raises(gpu.AqzError) as e:
        rd.load_frames(data, off, None, code, stream_ptr=_stream())
    assert e.value.status == 1 and gpu.lib().aqz_last_error()
    rd.load_frames_region(data, off, 0, 2, region, None, code, stream_ptr=_stream())
    assert rd.status()[1] == 0
    assert np.array_equal(read_crop(rd, 0, 2, region, 2), crop_bytes(frames, 0, 2, region))
    rd.close()
    # one byte less and the region load is refused too
    rd = gpu.Reader(SEL, U16, codecs=gpu.DECODE_CODEC_LZ4, max_frames_bytes=needed - 1)
    with pytest.raises(gpu.AqzError) as e:
        rd.load_frames_region(data, off, 0, 2, region, None, code, stream_ptr=_stream())
    assert e.value.status == 1
    rd.close()


def test_window_of_a_region_load(gpu):
    """A read inside the loaded window is exact; one that needs a chunk more, and a
    read_frames, are refused on the host with a text that names the window, and
    nothing is enqueued.  The next full load lifts the window."""
    torch = _torch()
    frames, layers = selective_inputs(gpu)
    code, data, off, entries = layers["lz4"]
    region, want_set = SEL_REGIONS["corner"]
    rd = gpu.Reader(SEL, U16, codecs=gpu.DECODE_CODEC_LZ4)
    rd.load_frames_region(data, off, 0, 2, region, None, code, stream_ptr=_stream())
    for sub in ((29, 27, 3, 5), (33, 34, 4, 3), (0, 0, 64, 64), region):
        for first, count in frame_ranges(2):
            assert np.array_equal(read_crop(rd, first, count, sub, 2),
                                  crop_bytes(frames, first, count, sub)), sub
    fb = rd.layout()["frame_bytes"]
    dst = torch.full((2 * fb,), FILL, dtype=torch.uint8, device="cuda")

    def refused(call):
        with pytest.raises(gpu.AqzError) as e:
            call()
        assert e.value.status == 1
        text = gpu.lib().aqz_last_error().decode()
        assert "window" in text and "x0 29" in text and "width 9" in text, text

    # one pixel into tile column 2: chunk 2 was not loaded
    refused(lambda: rd.read_region_ptr(0, 1, (29, 27, 36, 1), dst.data_ptr(), 96 * 2, fb,
                                       _stream()))
    refused(lambda: rd.read_frames_ptr(0, 1, dst.data_ptr(), fb, _stream()))
    refused(lambda: rd.read_frames_ptr(0, 2, dst.data_ptr(), fb, _stream()))
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    # a full load lifts the window
    rd.load_frames(data, off, None, code, stream_ptr=_stream())
    assert np.array_equal(read_frames(rd, 0, 2), frames.view(np.uint8).reshape(2, -1))
    rd.close()


# ---- 4. a crop from shard bytes ------------------------------------------------------
def test_crop_gathered_from_shard_bytes(gpu):
    """tests/test_gpu_reader.py's test_frames_gathered_from_shard_bytes, fetching only
    the chunks of region_chunks by the pairs of aqz_shard_table_parse."""
    rng = np.random.default_rng(3)
    frames = camera_like(rng, 4 * 64 * 96, np.uint16).reshape(4, 64, 96)
    frames[:, 32:64, 32:64] = 0
    hole = 1 * 3 + 1
    st = gpu.Stage(SEL, U16, MEAN, multiscale=False, layer_slots=2, max_batch_frames=4)
    st.append(frames)
    st.synchronize()
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
    rd = gpu.Reader(SEL, U16, codecs=gpu.DECODE_CODEC_LZ4)
    unwritten = (1 << 64) - 1
    sub = (27, 33, 45, 7)                     # tiles (1, 0..2): the hole among them
    for layer in range(2):
        for first, count in frame_ranges(2):
            assert list(rd.region_chunks(first, count, (27, 29, 45, 7))) == [0, 1, 2, 3, 4, 5]
            need = rd.region_chunks(first, count, sub)
            assert list(need) == [3, 4, 5]
            parts, chunks = [], []
            for c in need:
                shard, internal = where[layer][int(c)]
                off, ext = int(tables[shard][0][internal]), int(tables[shard][1][internal])
                if c == hole:
                    assert off == ext == unwritten
                    continue
                parts.append(blobs[shard][off:off + ext])
                chunks.append(int(c))
            blob = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
            offs = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
            rd.load_frames_region(blob, offs, first, count, sub, chunks, gpu.CODEC_BLOSC_LZ4,
                                  stream_ptr=_stream())
            status, bad = rd.status()
            assert bad == 0 and status[hole] == SKIPPED
            assert (status[[3, 5]] == OK).all() and (status[:3] == NOT_LOADED).all()
            want = crop_bytes(frames[2 * layer:2 * layer + 2], first, count, sub)
            assert np.array_equal(read_crop(rd, first, count, sub, 2), want)
    rd.close()
    st.close()


# ---- 5. damage inside the window ----------------------------------------------------
def test_damaged_frame_inside_the_window(gpu):
    """The mutation tests/test_gpu_reader.py pins as CORRUPT (match_offset_0 of the
    camera_ts4_sh1 golden frame), applied to one frame inside the window: that chunk
    gets the status, the window's other chunks are exact, the chunks outside it are
    NOT_LOADED, and read_crop asserts that nothing outside the crop's rows changed."""
    torch = _torch()
    golden = {name: fr for name, fr, *_ in load_golden()}["camera_ts4_sh1"]
    name, damaged, chunk_bytes, want_status = next(
        m for m in named_mutations(golden) if m[0] == "match_offset_0")
    assert want_status == CORRUPT and chunk_bytes == 3000
    dims = [(TIME, 0, 3, 1), (SPACE, 12, 5, 1), (SPACE, 100, 50, 1)]   # 3 x 2 tiles
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
    victim = 1 * 2 + 1
    parts = [bytes(data[o[c]:o[c + 1]]) for c in range(n)]
    parts[victim] = damaged
    blob = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    offs = np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)
    region = (41, 3, 31, 5)                    # rows 3-7, pixels 41-71: tiles (0..1, 0..1)
    window = [0, 1, 2, 3]
    rd = gpu.Reader(dims, U32, codecs=gpu.DECODE_CODEC_LZ4)
    assert list(rd.region_chunks(0, F, region)) == window
    rd.load_frames_region(blob, offs, 0, F, region, list(range(n)), gpu.CODEC_BLOSC_LZ4,
                          stream_ptr=_stream())
    status, bad = rd.status()
    assert bad == 1 and status[victim] == CORRUPT
    assert (status[[0, 1, 2]] == OK).all() and (status[4:] == NOT_LOADED).all()
    x0, y0, w, h = region
    for packed in (False, True):
        got = read_crop(rd, 0, F, region, 4, packed).copy().view(np.uint32)
        want = frames[:, y0:y0 + h, x0:x0 + w].copy()
        # the victim's tile (ty 1, tx 1) inside the crop: rows 5-7, pixels 50-71
        got[:, 5 - y0:, 50 - x0:] = 0
        want[:, 5 - y0:, 50 - x0:] = 0
        assert np.array_equal(got, want)
    comp.close()
    rd.close()


# ---- 6. refusals -------------------------------------------------------------------
def test_region_refusals(gpu):
    torch = _torch()
    dims = GEOMETRIES["ragged"]                 # 45 rows of 70 u16 pixels, 3 frames a layer
    od = OracleDims(dims, U16)
    rd = gpu.Reader(dims, U16, codecs=gpu.DECODE_CODEC_LZ4)
    n, bpc = od.number_of_chunks_in_memory(), od.bytes_per_chunk()
    dst = torch.full((3 * 45 * 70 * 2,), FILL, dtype=torch.uint8, device="cuda")
    ok = (3, 5, 20, 10)

    def refused(call):
        with pytest.raises(gpu.AqzError) as e:
            call()
        assert e.value.status == 1
        assert gpu.lib().aqz_last_error()

    def read(first, count, region, rs=40, fs=None):
        fs = 9 * rs + 40 if fs is None else fs
        return lambda: rd.read_region_ptr(first, count, region, dst.data_ptr(), rs, fs,
                                          _stream())

    refused(read(0, 1, ok))                                   # a read before any load
    blob = np.zeros(n * bpc, dtype=np.uint8)
    off = np.arange(n + 1, dtype=np.uint64) * bpc
    order = list(range(n))

    def load(first, count, region):
        return lambda: rd.load_frames_region(blob, off, first, count, region, order,
                                             gpu.CODEC_NONE, stream_ptr=_stream())

    bad_regions = [None, (3, 5, 0, 10), (3, 5, 20, 0), (0xffffffff, 5, 2, 10),
                   (3, 0xffffffff, 20, 2), (51, 5, 20, 10), (3, 36, 20, 10)]
    for region in bad_regions:
        refused(load(0, 1, region))
        refused(lambda: rd.region_chunks(0, 1, region))
    for first, count in ((0, 0), (3, 1), (2, 2), (0xffffffff, 2)):
        refused(load(first, count, ok))                       # a range outside the layer
        refused(lambda: rd.region_chunks(first, count, ok))
    refused(read(0, 1, ok))                                   # still nothing loaded
    load(0, 3, (0, 0, 70, 45))()
    for region in bad_regions:
        refused(read(0, 1, region))
    for first, count in ((0, 0), (3, 1), (2, 2), (0xffffffff, 2)):
        refused(read(first, count, ok))
    refused(read(0, 1, ok, rs=39))                            # a row stride too small
    refused(read(0, 1, ok, rs=40, fs=9 * 40 + 39))            # a frame stride too small
    refused(read(0, 2, ok, rs=47, fs=9 * 47 + 39))
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == FILL).all()
    # the smallest strides are taken, and stored chunks of zeros read as zeros
    read(1, 2, ok, rs=40, fs=9 * 40 + 40)()
    torch.cuda.synchronize()
    b = dst.cpu().numpy()
    assert not b[:2 * 400].any() and (b[2 * 400:] == FILL).all()
    rd.close()
