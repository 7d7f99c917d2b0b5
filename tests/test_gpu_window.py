"""GPU tests of the ranged decode (aqz_decompressor_run_ranges) and of the window
load built on it (aqz_reader_load_frames_window, aqz_reader_load_stats).

A ranged run decodes, of every frame, only the blosc blocks that meet a byte range of
the chunk.  Each check paints the destination with 0xA5 and asks three things of a
(frame, range): the bytes of the reported span are the payload's (a byte mover: no
tolerance), the span is the block-aligned interval of the range -- computed here from
the frame's own header (codec_helpers.header) -- and every byte outside it still holds
the paint.  The reference payload is the full aqz_decompressor_run."""
import numpy as np
import pytest

from codec_helpers import camera_like, header
from decoder_helpers import (BAD_HEADER, CORRUPT, MUTATED, OK, SKIPPED, UNSUPPORTED,
                             load_golden, named_mutations, sha256, streams)
from oracle_bindings import NP_DTYPES, SPACE, TIME, U8, U16, U32, U64, OracleDims
from region_helpers import (GEOMETRIES, PERMUTED, XY_ORDER, XY_SHAPES, frame_ranges,
                            regions_of, xy_dims)

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
NOT_LOADED = 5
LDS_BYTES = 32 * 1024          # kDecodeLdsBytes: larger blocks take the scratch path
ZSTD_MAX_PASSES = 8            # kZstdMaxPasses
BY_SIZE = {1: U8, 2: U16, 4: U32, 8: U64}
DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def _torch():
    import torch
    return torch


def _stream():
    return _torch().cuda.current_stream().cuda_stream


# ---- the range math, restated from the frame's header ---------------------------------
def geometry_of(frame):
    """(nbytes, blocksize, nblocks, memcpyed) of a blosc1 frame"""
    h = header(frame)
    return h["nbytes"], h["blocksize"], -(-h["nbytes"] // h["blocksize"]), bool(h["flags"] & 2)


def span_of(frame, lo, hi):
    """What a ranged decode of chunk bytes [lo, hi) of this frame reports: the blocks
    [lo // blocksize, ceil(hi / blocksize)) clipped to nblocks, as bytes; exactly
    [lo, hi) for a memcpyed frame (it has no blocks); (0, 0) for an empty range."""
    nb, bs, nblocks, memcpyed = geometry_of(frame)
    if lo == hi:
        return 0, 0
    if memcpyed:
        return lo, hi
    jlo, jhi = lo // bs, min(-(-hi // bs), nblocks)
    return jlo * bs, min(jhi * bs, nb)


def ranges_of(frame):
    """{name: (lo, hi)}: the ranges every frame is checked with."""
    nb, bs, nblocks, _ = geometry_of(frame)
    last0 = (nblocks - 1) * bs                  # first byte of the last (or leftover) block
    out = {
        "first-byte": (0, 1),
        "last-byte": (nb - 1, nb),
        # over the first block edge; a frame of one block has none: its last two bytes
        "block-edge": (min(bs, nb - 1) - 1, min(bs, nb - 1) + 1),
        # from the block before it (where there is one) to the middle of the last block
        "ends-in-last-block": (max(last0 - 1, 0), last0 + max((nb - last0) // 2, 1)),
        "whole": (0, nb),
        "empty": (nb // 2, nb // 2),
    }
    assert all(0 <= lo <= hi <= nb for lo, hi in out.values())
    return out


class Ranged:
    def __init__(self, chunks, status, spans, pads_untouched):
        self.chunks, self.status, self.spans = chunks, status, spans
        self.pads_untouched = pads_untouched


def upload_frames(frames):
    torch = _torch()
    blob = b"".join(frames)
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)
    fd = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to("cuda")
    return fd, len(blob), torch.from_numpy(off).to("cuda")


def run_full(dec, frames, chunk_bytes):
    """aqz_decompressor_run of the frames -> (chunks, status)"""
    torch = _torch()
    fd, nbytes, od = upload_frames(frames)
    n = len(frames)
    dst = torch.full((n * chunk_bytes,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x7f, dtype=torch.int32, device="cuda")
    dec.run_ptr(fd.data_ptr(), nbytes, od.data_ptr(), n, dst.data_ptr(), chunk_bytes,
                chunk_bytes, status.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dst.cpu().numpy().reshape(n, chunk_bytes), status.cpu().numpy().astype(np.uint32)


def run_ranged(dec, frames, chunk_bytes, ranges, pad=24, spans=True):
    """aqz_decompressor_run_ranges of frame i over ranges[i] into a FILL-painted
    destination of pitch chunk_bytes + pad with a guard behind the last chunk."""
    torch = _torch()
    fd, nbytes, od = upload_frames(frames)
    n = len(frames)
    pitch = chunk_bytes + pad
    dst = torch.full((n * pitch + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x7f, dtype=torch.int32, device="cuda")
    rg = torch.from_numpy(np.array(ranges, dtype=np.int64).reshape(n, 2)).to("cuda")
    sp = torch.full((n, 2), 0x7777, dtype=torch.int64, device="cuda")
    dec.run_ranges_ptr(fd.data_ptr(), nbytes, od.data_ptr(), n, dst.data_ptr(), pitch,
                       chunk_bytes, rg.data_ptr(), sp.data_ptr() if spans else None,
                       status.data_ptr(), _stream())
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    body = d[:n * pitch].reshape(n, pitch)
    untouched = bool((body[:, chunk_bytes:] == FILL).all() and (d[n * pitch:] == FILL).all())
    return Ranged(body[:, :chunk_bytes], status.cpu().numpy().astype(np.uint32),
                  sp.cpu().numpy().astype(np.uint64), untouched)


def check_one(got, i, payload, lo, hi, span, what):
    """Chunk i of a ranged run against its payload: status, span, bytes, paint."""
    nb = len(payload)
    want_status = NOT_LOADED if lo == hi else OK
    assert got.status[i] == want_status, (what, got.status[i])
    assert tuple(int(v) for v in got.spans[i]) == span, (what, got.spans[i], span)
    s0, s1 = span
    assert s0 <= lo and hi <= s1 or lo == hi, what
    chunk = got.chunks[i]
    assert chunk[s0:s1].tobytes() == payload[s0:s1], (what, "bytes of the span")
    assert chunk[lo:hi].tobytes() == payload[lo:hi], (what, "bytes of the range")
    outside = np.ones(nb, dtype=bool)
    outside[s0:s1] = False
    assert (chunk[outside] == FILL).all(), (what, "a byte outside the span was written")


def check_frame(dec, frame, payload, what, extra=()):
    """One run with a copy of the frame per range of ranges_of (and the extra ones);
    the whole-chunk range must also give what the full run gave."""
    nb = len(payload)
    ranges = dict(ranges_of(frame))
    ranges.update(extra)
    names = list(ranges)
    got = run_ranged(dec, [frame] * len(names), nb, [ranges[k] for k in names])
    assert got.pads_untouched, what
    for i, name in enumerate(names):
        lo, hi = ranges[name]
        check_one(got, i, payload, lo, hi, span_of(frame, lo, hi), (what, name, lo, hi))
    return got, names


# ---- 1. golden c-blosc frames -----------------------------------------------------------
def test_golden_cblosc_frames_by_range(gpu):
    golden = load_golden()
    groups = {}
    for name, fr, _, _, digest in golden:
        groups.setdefault(header(fr)["nbytes"], []).append((name, fr, digest))
    # the fixture holds what the ranges are about: a memcpyed frame, blocks above the
    # LDS budget (the scratch path), a leftover block, frames of several blocks
    geo = {name: geometry_of(fr) for name, fr, *_ in golden}
    assert any(m for *_, m in geo.values())
    assert any(bs > LDS_BYTES and not m for _, bs, _, m in geo.values())
    assert geo["long_streams"][1] > LDS_BYTES
    assert any(nb % bs and nblocks > 1 and not m for nb, bs, nblocks, m in geo.values())
    dec = gpu.Decompressor(max(groups), max(8, max(len(g) for g in groups.values())))
    for nbytes, items in sorted(groups.items()):
        frames = [fr for _, fr, _ in items]
        ref, st = run_full(dec, frames, nbytes)
        for i, (name, fr, digest) in enumerate(items):
            assert st[i] == OK and sha256(ref[i].tobytes()) == digest, name
            got, names = check_frame(dec, fr, ref[i].tobytes(), name)
            whole = names.index("whole")
            assert np.array_equal(got.chunks[whole], ref[i]), name
    # spans are optional
    name, fr, *_ = golden[0]
    nb = header(fr)["nbytes"]
    got = run_ranged(dec, [fr], nb, [(0, nb)], spans=False)
    ref, _ = run_full(dec, [fr], nb)
    assert got.status[0] == OK and np.array_equal(got.chunks[0], ref[0])
    assert (got.spans == 0x7777).all()
    dec.close()


# ---- 2. this library's frames -----------------------------------------------------------
def pixels(rng, n_px, ts):
    """camera-like pixels of ts bytes; the 8-bit ones dimmer, so that they do not clip,
    and without noise, so that LZ4 still finds matches in unshuffled bytes"""
    if ts == 1:
        return camera_like(rng, n_px, np.uint8, level=120.0, noise=0.0, amp=40.0)
    return camera_like(rng, n_px, DT[ts])


def compress(gpu, chunks, ts, codec, clevel, shuffle):
    """chunks (n, nb) uint8 -> the list of their frames, made on the device."""
    torch = _torch()
    n, nb = chunks.shape
    src = torch.from_numpy(np.ascontiguousarray(chunks)).to("cuda")
    comp = gpu.Compressor(nb, ts, codec=codec, clevel=clevel, shuffle=shuffle)
    cap = comp.max_bytes(n)
    fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(), _stream())
    torch.cuda.synchronize()
    comp.close()
    o, f = off.cpu().numpy(), fr.cpu().numpy()
    return [f[o[i]:o[i + 1]].tobytes() for i in range(n)]


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_library_lz4_frames_by_range(gpu, ts, shuffle):
    """About 80 KiB and a ragged tail: 20 and 10 blocks of the library's 4096 * ts bytes
    for ts 1 and 2.  For ts 4 and 8 (16 and 32 KiB blocks) 80 KiB holds 5 and 2, so the
    chunk grows to 9 blocks and a half: at least 9 blocks and a leftover for every ts,
    and a range that starts in the third LDS group of the workgroup's walk."""
    bs = 4096 * ts
    nb = max(80 * 1024, 9 * bs) + bs // 2 + 37 * ts
    rng = np.random.default_rng(100 * ts + shuffle)
    payload = pixels(rng, nb // ts, ts).view(np.uint8)
    frame, = compress(gpu, payload[None, :], ts, gpu.CODEC_BLOSC_LZ4, 5, shuffle)
    g_nb, g_bs, nblocks, memcpyed = geometry_of(frame)
    assert (g_nb, g_bs) == (nb, bs) and nblocks >= 9 + 1 and nb % bs and not memcpyed
    group = min(8, LDS_BYTES // ((bs + 15) & ~15))     # blocks a workgroup takes at a time
    assert nblocks > 2 * group
    third = 2 * group * bs
    dec = gpu.Decompressor(nb, 16)
    ref, st = run_full(dec, [frame], nb)
    assert st[0] == OK and ref[0].tobytes() == payload.tobytes()
    got, names = check_frame(dec, frame, payload.tobytes(), (ts, shuffle),
                             extra={"third-group": (third + 1, third + 4),
                                    "two-groups": (third - 1, min(third + group * bs + 1, nb))})
    assert np.array_equal(got.chunks[names.index("whole")], ref[0])
    dec.close()


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_library_blosc_zstd_frames_by_range(gpu, ts, shuffle):
    """9 full 256 KiB blocks and a leftover: more blocks than the decoder has passes.
    A plain zstd frame of the same payload rides in the same run: its span is the whole
    chunk whatever its range, and its bytes are exact."""
    bs = 256 * 1024
    nb = 9 * bs + 40_000 + 8 * 3
    rng = np.random.default_rng(200 * ts + shuffle)
    payload = pixels(rng, nb // ts, ts).view(np.uint8)
    frame, = compress(gpu, payload[None, :], ts, gpu.CODEC_BLOSC_ZSTD, 3, shuffle)
    plain, = compress(gpu, payload[None, :], ts, gpu.CODEC_ZSTD, 3, 0)
    g_nb, g_bs, nblocks, memcpyed = geometry_of(frame)
    assert (g_nb, g_bs) == (nb, bs) and nblocks == 10 > ZSTD_MAX_PASSES and not memcpyed
    assert plain[:4] == b"\x28\xb5\x2f\xfd"
    variants = [gpu.DECODE_CODEC_ZSTD]
    if (ts, shuffle) == (2, 1):
        variants.append(gpu.DECODE_CODEC_ZSTD | gpu.DECODE_ZSTD_PARALLEL)
    for codecs in variants:
        dec = gpu.Decompressor(nb, 16, codecs)
        ref, st = run_full(dec, [frame, plain], nb)
        assert (st == OK).all() and ref[0].tobytes() == payload.tobytes()
        assert ref[1].tobytes() == payload.tobytes()
        ranges = ranges_of(frame)
        names = list(ranges)
        frames = [frame] * len(names) + [plain, plain]
        rg = [ranges[k] for k in names] + [(5, 6), (0, 0)]
        got = run_ranged(dec, frames, nb, rg)
        assert got.pads_untouched
        for i, name in enumerate(names):
            lo, hi = ranges[name]
            check_one(got, i, payload.tobytes(), lo, hi, span_of(frame, lo, hi),
                      (ts, shuffle, codecs, name))
        assert np.array_equal(got.chunks[names.index("whole")], ref[0])
        k = len(names)
        assert got.status[k] == OK and tuple(got.spans[k]) == (0, nb)
        assert np.array_equal(got.chunks[k], ref[1])
        # an empty range: not decoded, whatever the frame's kind
        assert got.status[k + 1] == NOT_LOADED and tuple(got.spans[k + 1]) == (0, 0)
        assert (got.chunks[k + 1] == FILL).all()
        dec.close()


def test_skipped_and_mixed_frames_by_range(gpu):
    """A zero-length frame is zero-filled over its range only; LZ4 frames given to a
    decoder without the codec keep their status."""
    nb = 3 * 4096 + 100
    rng = np.random.default_rng(5)
    payload = camera_like(rng, nb // 2, np.uint16).view(np.uint8)
    frame, = compress(gpu, payload[None, :], 2, gpu.CODEC_BLOSC_LZ4, 5, 1)
    dec = gpu.Decompressor(nb, 8)
    got = run_ranged(dec, [b"", b"", frame, b""], nb, [(7, 4100), (0, 0), (0, nb), (3, nb)])
    assert got.pads_untouched
    assert list(got.status) == [SKIPPED, NOT_LOADED, OK, SKIPPED]
    assert [tuple(s) for s in got.spans.tolist()] == [(7, 4100), (0, 0), (0, nb), (3, nb)]
    assert not got.chunks[0][7:4100].any() and (got.chunks[0][:7] == FILL).all()
    assert (got.chunks[0][4100:] == FILL).all() and (got.chunks[1] == FILL).all()
    assert got.chunks[2].tobytes() == payload.tobytes()
    assert not got.chunks[3][3:].any() and (got.chunks[3][:3] == FILL).all()
    dec.close()
    zdec = gpu.Decompressor(nb, 8, gpu.DECODE_CODEC_ZSTD)
    got = run_ranged(zdec, [frame], nb, [(0, nb)])
    assert got.status[0] == UNSUPPORTED and (got.chunks[0] == FILL).all()
    zdec.close()


# ---- 3. defects -------------------------------------------------------------------------
def _block_of_defect(good, bad):
    """The block whose table entry or records hold the first byte in which the
    mutated frame differs from the good one; None for a defect in the 16-byte header
    or a changed length (the header is read for every range)."""
    if len(bad) != len(good):
        return None
    at = next(i for i in range(len(good)) if good[i] != bad[i])
    if at < 16:
        return None
    nb, bs, nblocks, _ = geometry_of(good)
    if at < 16 + 4 * nblocks:
        return (at - 16) // 4
    for j, _, pos, cs, _ in streams(good):
        if pos <= at < pos + 4 + cs:
            return j
    raise AssertionError("the defect lies in no block")


# golden frames of several blocks (MUTATED's camera frames have one): split streams with
# a leftover block, bit-shuffled ones, and 256 KiB streams
SEVERAL_BLOCKS = ("split_two_full_and_leftover", "split_bitshuffle_leftover", "long_streams")


@pytest.mark.parametrize("source", SEVERAL_BLOCKS)
def test_defects_inside_and_outside_the_span(gpu, source):
    """decoder_helpers.named_mutations of a golden frame.  A defect inside a block --
    its table entry, a record's size, its LZ4 stream -- is the mutation's own status
    for a range that meets the block, and is not looked at (status OK, exact bytes, the
    paint outside the span) for a range inside another block.  The mutations of the
    16-byte header and of the frame's length are found by the header check every
    non-empty range makes: they keep their status for both ranges.  A range with hi >
    chunk_bytes is BAD_HEADER and writes nothing."""
    good = {name: fr for name, fr, *_ in load_golden()}[source]
    nb, bs, nblocks, _ = geometry_of(good)
    assert nblocks >= 2 and "long_streams" in MUTATED
    dec = gpu.Decompressor(nb, 64)
    ref, st = run_full(dec, [good], nb)
    assert st[0] == OK
    payload = ref[0].tobytes()
    muts = named_mutations(good)
    last = ((nblocks - 1) * bs + 1, nb)          # inside the last block
    first = (1, min(bs, nb) - 1)                 # inside block 0
    frames, ranges, expect = [], [], []
    in_a_block = 0
    for name, data, cb, status in muts:
        assert cb == nb
        j = _block_of_defect(good, data)
        for rng_name, r, block in (("last", last, nblocks - 1), ("first", first, 0)):
            frames.append(data)
            ranges.append(r)
            expect.append((name, rng_name, status if j is None or j == block else OK))
        in_a_block += j is not None
        frames.append(data)
        ranges.append((0, nb + 1))
        expect.append((name, "past-the-chunk", BAD_HEADER))
    # the defects of the first LZ4 stream lie in block 0; one lies in the last block
    assert in_a_block >= 6 and {BAD_HEADER, CORRUPT, UNSUPPORTED} <= {m[3] for m in muts}
    got = run_ranged(dec, frames, nb, ranges)
    assert got.pads_untouched
    seen = set()
    for i, (name, rng_name, status) in enumerate(expect):
        lo, hi = ranges[i]
        what = (name, rng_name)
        assert got.status[i] == status, (what, got.status[i], status)
        if rng_name == "past-the-chunk":
            assert (got.chunks[i] == FILL).all() and tuple(got.spans[i]) == (0, 0), what
        elif status == OK:
            check_one(got, i, payload, lo, hi, span_of(good, lo, hi), what)
            seen.add(rng_name)
        else:
            # nothing outside the span the range asks for is written, whatever it holds
            s0, s1 = span_of(good, lo, hi)
            assert (got.chunks[i][:s0] == FILL).all() and (got.chunks[i][s1:] == FILL).all(), what
    assert seen == {"last", "first"}
    dec.close()


# ---- 4. the reader ----------------------------------------------------------------------
def make_layer(gpu, dims, order, dtype, seed):
    """One layer of frames in acquisition order and its chunks (n, bpc) as the oracle's
    write path lays them out through the storage order."""
    d = gpu.Dims(dims, dtype, storage_order=order)
    storage = [dims[i] for i in order] if order else dims
    xy = order is not None and order[-2:] != [len(dims) - 2, len(dims) - 1]
    od = OracleDims(storage, dtype)
    F, n, bpc = od.frames_per_chunk_layer(), od.number_of_chunks_in_memory(), od.bytes_per_chunk()
    H, W = dims[-2][1], dims[-1][1]
    # camera-like pixels compress: the frames keep their blocks (random ones are memcpyed)
    rng = np.random.default_rng(seed)
    frames = camera_like(rng, F * H * W, NP_DTYPES[dtype]).reshape(F, H, W)
    buf, has = od.new_layer()
    for f in range(F):
        sframe = np.ascontiguousarray(frames[f].T) if xy else frames[f]
        od.write_frame_to_chunks(d.transpose_frame_id(f), sframe, buf, has)
    assert has.all()
    return frames, buf.reshape(n, bpc), xy


def layer_frames(gpu, chunks, ts, codec, shuffle):
    """-> (frames blob uint8, offsets uint64, list of frames) in chunk order"""
    n, bpc = chunks.shape
    if codec == gpu.CODEC_NONE:
        frames = [chunks[c].tobytes() for c in range(n)]
    else:
        frames = compress(gpu, chunks, ts, codec, 5 if codec == gpu.CODEC_BLOSC_LZ4 else 3,
                          shuffle)
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.uint64)
    return np.frombuffer(b"".join(frames), dtype=np.uint8).copy(), off, frames


def read_crop(rd, first, count, region, bpp):
    """The crop into a FILL-painted buffer at an odd base with padded strides; every
    byte outside the crop's rows must keep the fill.  -> (count, height, width * bpp)"""
    torch = _torch()
    x0, y0, w, h = region
    rb = w * bpp
    base, rs = 3, rb + 5
    fs = (h - 1) * rs + rb + 7
    buf = torch.full((base + count * fs + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    rd.read_region_ptr(first, count, region, buf.data_ptr() + base, rs, fs, _stream())
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    at = (base + np.arange(count)[:, None, None] * fs + np.arange(h)[None, :, None] * rs +
          np.arange(rb)[None, None, :])
    outside = np.ones(len(b), dtype=bool)
    outside[at.ravel()] = False
    assert (b[outside] == FILL).all(), "bytes outside the crop's rows changed"
    return b[at]


def crop_bytes(frames, first, count, region):
    x0, y0, w, h = region
    c = np.ascontiguousarray(frames[first:first + count, y0:y0 + h, x0:x0 + w])
    return c.view(np.uint8).reshape(count, h, -1)


def refused(fn, *args):
    """The call is AQZ_STATUS_INVALID_ARGUMENT and its text names the window."""
    import aqz
    with pytest.raises(aqz.AqzError) as e:
        fn(*args)
    assert e.value.status == 1 and "outside the loaded window" in str(e.value), str(e.value)


def predicted_decoded_bytes(rd, frames, first, count, region, plain):
    """The sum of the spans the range functions predict for a window load."""
    chunks, ranges = rd.region_chunk_ranges(first, count, region)
    total = 0
    for c, (lo, hi) in zip(chunks.tolist(), ranges.tolist()):
        if plain:
            total += rd.layout()["bytes_per_chunk"]
        else:
            s0, s1 = span_of(frames[c], lo, hi)
            total += s1 - s0
    return total


def check_window_loads(gpu, rd, dims, dtype, frames, blob, off, frame_list, codec, mem, xy,
                       plain=False, regions=None, ranges=None):
    """load_frames_window + read_region for every region x frame range against the numpy
    crop, with the statuses, the stats and the refusals of the exact window."""
    torch = _torch()
    ts = np.dtype(NP_DTYPES[dtype]).itemsize
    lay = rd.layout()
    F, n, bpc = lay["frames_per_layer"], lay["chunks_per_layer"], lay["bytes_per_chunk"]
    H, W = dims[-2][1], dims[-1][1]
    src = torch.from_numpy(blob).to("cuda") if mem == "device" else blob
    cof = np.arange(n, dtype=np.uint32)
    all_regions = regions_of(dims, "x" if xy else "y")
    for name in regions or all_regions:
        region = all_regions[name]
        for first, count in ranges or frame_ranges(F):
            rd.load_frames_window(src, off, first, count, region, cof, codec,
                                  stream_ptr=_stream())
            what = (name, region, first, count)
            got = read_crop(rd, first, count, region, ts)
            assert np.array_equal(got, crop_bytes(frames, first, count, region)), what
            status, bad = rd.status()
            inside = rd.region_chunks(first, count, region)
            assert bad == 0 and np.isin(status[inside], (OK, SKIPPED)).all(), (what, status)
            assert (np.delete(status, inside) == NOT_LOADED).all(), (what, status)
            decoded, copied = rd.load_stats()
            if codec != gpu.CODEC_NONE:
                assert decoded == predicted_decoded_bytes(rd, frame_list, first, count, region,
                                                          plain), what
                assert copied == sum(len(frame_list[c]) for c in inside), what
            else:
                assert decoded == 0
            # one frame, one pixel more: refused, nothing enqueued, the paint intact
            x0, y0, w, h = region
            wider = [(x0 - 1, y0, w + 1, h)] if x0 else []
            wider += [(x0, y0, w + 1, h)] if x0 + w < W else []
            wider += [(x0, y0, w, h + 1)] if y0 + h < H else []
            dst = torch.full((count + 1, H * W * ts), FILL, dtype=torch.uint8, device="cuda")
            for r in wider:
                refused(rd.read_region_ptr, first, count, r, dst.data_ptr(), r[2] * ts,
                        r[2] * r[3] * ts, _stream())
            if first + count < F:
                refused(rd.read_region_ptr, first, count + 1, region, dst.data_ptr(), w * ts,
                        w * h * ts, _stream())
                refused(rd.read_frames_ptr, first, count + 1, dst.data_ptr(), H * W * ts,
                        _stream())
            if first:
                refused(rd.read_region_ptr, first - 1, 1, region, dst.data_ptr(), w * ts,
                        w * h * ts, _stream())
            if region != all_regions["whole"]:
                refused(rd.read_frames_ptr, first, count, dst.data_ptr(), H * W * ts, _stream())
            torch.cuda.synchronize()
            assert bool((dst == FILL).all()), what
    # a later full load restores full reads
    rd.load_frames(src, off, cof, codec, stream_ptr=_stream())
    fb = lay["frame_bytes"]
    buf = torch.empty(F * fb, dtype=torch.uint8, device="cuda")
    rd.read_frames_ptr(0, F, buf.data_ptr(), fb, _stream())
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == frames.tobytes()
    status, bad = rd.status()
    assert bad == 0 and (status == OK).all()
    decoded, copied = rd.load_stats()
    assert decoded == (n * bpc if codec != gpu.CODEC_NONE else 0)
    assert copied == (len(blob) if mem == "host" else 0)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_window_load_every_geometry_lz4(gpu, geometry, mem):
    dims, dtype = GEOMETRIES[geometry], U16
    frames, chunks, xy = make_layer(gpu, dims, None, dtype, 300)
    blob, off, frame_list = layer_frames(gpu, chunks, 2, gpu.CODEC_BLOSC_LZ4, 1)
    rd = gpu.Reader(dims, dtype, codecs=gpu.DECODE_CODEC_LZ4)
    check_window_loads(gpu, rd, dims, dtype, frames, blob, off, frame_list,
                       gpu.CODEC_BLOSC_LZ4, mem, xy)
    rd.close()


STORAGE = {
    "aligned": (GEOMETRIES["aligned"], None),
    "5d": (GEOMETRIES["5d"], None),
    "5d-permuted": PERMUTED,
    "xy-45x70": (xy_dims(XY_SHAPES[1]), XY_ORDER),
}
CODECS = {
    # name: (codec, shuffle, reader codecs, plain)
    "none": ("CODEC_NONE", 0, "lz4", False),
    "lz4-bitshuffle": ("CODEC_BLOSC_LZ4", 2, "lz4", False),
    "blosc-zstd": ("CODEC_BLOSC_ZSTD", 1, "zstd", False),
    "zstd": ("CODEC_ZSTD", 0, "zstd", True),
    "zstd-parallel": ("CODEC_ZSTD", 0, "zstd-parallel", True),
}


def _reader_codecs(gpu, name):
    return {"lz4": gpu.DECODE_CODEC_LZ4, "zstd": gpu.DECODE_CODEC_ZSTD,
            "zstd-parallel": gpu.DECODE_CODEC_ZSTD | gpu.DECODE_ZSTD_PARALLEL}[name]


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("codec", list(CODECS))
@pytest.mark.parametrize("storage", list(STORAGE))
def test_window_load_codecs_and_storage_orders(gpu, storage, codec, mem):
    dims, order = STORAGE[storage]
    code, shuffle, rc, plain = CODECS[codec]
    code = getattr(gpu, code)
    frames, chunks, xy = make_layer(gpu, dims, order, U16, 310)
    blob, off, frame_list = layer_frames(gpu, chunks, 2, code, shuffle)
    rd = gpu.Reader(dims, U16, storage_order=order, codecs=_reader_codecs(gpu, rc))
    check_window_loads(gpu, rd, dims, U16, frames, blob, off, frame_list, code, mem, xy,
                       plain=plain)
    rd.close()


BLOCKY = {
    # a chunk of 8 * 48 * 64 * 2 = 49,152 bytes: 6 lz4 blocks of 8 KiB
    "lz4-6-blocks": ([(TIME, 0, 8, 1), (SPACE, 96, 48, 1), (SPACE, 128, 64, 1)],
                     "CODEC_BLOSC_LZ4", "lz4"),
    # a chunk of 28 * 128 * 128 * 2 = 917,504 bytes: 3 blosc-zstd blocks of 256 KiB and
    # a leftover
    "zstd-3-blocks": ([(TIME, 0, 28, 1), (SPACE, 256, 128, 1), (SPACE, 256, 128, 1)],
                      "CODEC_BLOSC_ZSTD", "zstd"),
}


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("case", list(BLOCKY))
def test_window_load_skips_blocks(gpu, case, mem):
    """Chunks of several blocks, a single middle frame: the load decodes the sum of the
    spans the range functions predict, and that is less than the window's chunks hold.
    It is the condition that shows work was skipped -- a cap, not a timing."""
    dims, code, rc = BLOCKY[case]
    code = getattr(gpu, code)
    frames, chunks, xy = make_layer(gpu, dims, None, U16, 320)
    n, bpc = chunks.shape
    blob, off, frame_list = layer_frames(gpu, chunks, 2, code, 1)
    for fr in frame_list:
        nb, bs, nblocks, memcpyed = geometry_of(fr)
        assert nb == bpc and not memcpyed
        if case == "lz4-6-blocks":
            assert bpc == 49_152 and nblocks >= 6
        else:
            assert bpc == 917_504 and bs == 256 * 1024 and nblocks == 4 and nb % bs
    rd = gpu.Reader(dims, U16, codecs=_reader_codecs(gpu, rc))
    F = rd.layout()["frames_per_layer"]
    mid = [(F // 2, 1)]
    names = ("row", "inside-a-tile", "corner")
    check_window_loads(gpu, rd, dims, U16, frames, blob, off, frame_list, code, mem, xy,
                       regions=names, ranges=mid)
    src = _torch().from_numpy(blob).to("cuda") if mem == "device" else blob
    cof = np.arange(n, dtype=np.uint32)
    all_regions = regions_of(dims)
    for name in names:
        region = all_regions[name]
        rd.load_frames_window(src, off, F // 2, 1, region, cof, code, stream_ptr=_stream())
        decoded, _ = rd.load_stats()
        inside = rd.region_chunks(F // 2, 1, region)
        want = predicted_decoded_bytes(rd, frame_list, F // 2, 1, region, False)
        print(case, name, "decoded", decoded, "predicted", want, "window chunks",
              len(inside) * bpc)
        assert decoded == want
        assert decoded < len(inside) * bpc
    rd.close()
