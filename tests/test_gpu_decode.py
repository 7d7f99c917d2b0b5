"""GPU tests of the device blosc1-LZ4 decoder (aqz_decompressor_*) and of the
stage's on-device write verification (aqz_stage_verify_layer): frames made by
the device compressor and by c-blosc 1.21 itself (tests/golden/
cblosc_lz4_frames.npz) decode on the device to exactly the chunk bytes, bytes
outside the chunks stay untouched, skipped / malformed / unsupported frames
get their status and leave their neighbours alone, and a stage verifies its
own compressed layers and reports a damaged copy of them."""
import numpy as np
import pytest

from codec_helpers import camera_like, chunk_payloads, header, oracle_decode
from decoder_helpers import (BAD_HEADER, CORRUPT, MUTATED, OK, SKIPPED, UNSUPPORTED,
                             load_golden, lz4_sequences, named_mutations, sha256, streams)
from oracle_bindings import MEAN, SPACE, TIME, U16, synthetic_frames

pytestmark = pytest.mark.gpu

DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
FILL = 0xA5
GUARD = 256
UINT32_MAX = (1 << 32) - 1


def _torch():
    import torch
    return torch


class Decoded:
    def __init__(self, chunks, status, pads_untouched):
        self.chunks, self.status, self.pads_untouched = chunks, status, pads_untouched


def run_decoder(gpu, dec, frames_dev, frames_bytes, off_dev, n, chunk_bytes, pad):
    """Decode n frames lying on the device into a FILL-painted destination of
    pitch chunk_bytes + pad with a guard region behind the last chunk."""
    torch = _torch()
    pitch = chunk_bytes + pad
    dst = torch.full((n * pitch + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x7f, dtype=torch.int32, device="cuda")
    dec.run_ptr(frames_dev.data_ptr(), frames_bytes, off_dev.data_ptr(), n, dst.data_ptr(),
                pitch, chunk_bytes, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    body = d[:n * pitch].reshape(n, pitch)
    untouched = bool((body[:, chunk_bytes:] == FILL).all() and (d[n * pitch:] == FILL).all())
    return Decoded(body[:, :chunk_bytes], status.cpu().numpy().astype(np.uint32), untouched)


def decode_host_frames(gpu, dec, frames, chunk_bytes, pad=24):
    """frames: list of bytes (b'' = skipped chunk), uploaded back to back."""
    torch = _torch()
    blob = b"".join(frames)
    off = np.cumsum([0] + [len(f) for f in frames]).astype(np.int64)
    fd = torch.from_numpy(np.frombuffer(blob + b"\0", dtype=np.uint8).copy()).to("cuda")
    od = torch.from_numpy(off).to("cuda")
    return run_decoder(gpu, dec, fd, len(blob), od, len(frames), chunk_bytes, pad)


def round_trip(gpu, chunks: np.ndarray, ts, clevel, shuffle, pad):
    """Compressor then Decompressor, the frames never leaving the device."""
    torch = _torch()
    n, nb = chunks.shape
    src = torch.from_numpy(np.ascontiguousarray(chunks)).to("cuda")
    comp = gpu.Compressor(nb, ts, clevel=clevel, shuffle=shuffle)
    cap = comp.max_bytes(n)
    fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    dec = gpu.Decompressor(nb, n)
    got = run_decoder(gpu, dec, fr, cap, off, n, nb, pad)
    dec.close()
    comp.close()
    assert (got.status == OK).all(), (ts, shuffle, nb, got.status)
    assert np.array_equal(got.chunks, chunks), (ts, shuffle, nb)
    assert got.pads_untouched, (ts, shuffle, nb)


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_round_trip_matrix(gpu, ts, shuffle):
    """The matrix of test_compressor_decodes_exactly, decoded on the device."""
    rng = np.random.default_rng(10 * ts + shuffle)
    for n_px in (16384, 40_000 // ts * 3, 1000, 50):
        pay = chunk_payloads(rng, DT[ts], n_px)
        chunks = np.stack([a.view(np.uint8) for a in pay.values()])
        round_trip(gpu, chunks, ts, 5, shuffle, pad=0 if n_px == 1000 else 40)


def test_round_trip_edge_sizes_and_pitch(gpu):
    """The edge list of test_compressor_edge_sizes_and_pitch, destination pitch
    above chunk_bytes (odd pads: unaligned chunk starts)."""
    rng = np.random.default_rng(3)
    for ts, n_px, pad in ((2, 16384 + 12000, 8), (4, 16384 * 2 + 9000, 48), (1, 13, 1),
                          (1, 12, 3), (2, 129, 5), (8, 127, 8), (1, 70_001, 16)):
        pay = chunk_payloads(rng, DT[ts], n_px, kinds=("camera", "random", "ramp"))
        chunks = np.stack([a.view(np.uint8) for a in pay.values()])
        for sh in (0, 1, 2):
            round_trip(gpu, chunks, ts, 5, sh, pad)


def test_round_trip_clevel0(gpu):
    rng = np.random.default_rng(4)
    chunks = np.stack([camera_like(rng, 20000, np.uint16).view(np.uint8) for _ in range(3)])
    round_trip(gpu, chunks, 2, 0, 1, pad=32)


def test_golden_cblosc_frames(gpu):
    """Every frame c-blosc made decodes to its payload: the sha256 recorded
    with it and the oracle's decode.  One run per chunk size."""
    groups = {}
    for name, fr, _, _, digest in load_golden():
        groups.setdefault(header(fr)["nbytes"], []).append((name, fr, digest))
    dec = gpu.Decompressor(max(groups), max(len(g) for g in groups.values()))
    for nbytes, items in sorted(groups.items()):
        got = decode_host_frames(gpu, dec, [fr for _, fr, _ in items], nbytes)
        assert got.pads_untouched, nbytes
        for i, (name, fr, digest) in enumerate(items):
            assert got.status[i] == OK, (name, got.status[i])
            data = got.chunks[i].tobytes()
            assert sha256(data) == digest, name
            assert data == oracle_decode(fr), name
    dec.close()


def test_skipped_chunks(gpu):
    rng = np.random.default_rng(6)
    nb = 2 * 5000
    chunks = [camera_like(rng, 5000, np.uint16).tobytes() for _ in range(3)]
    torch = _torch()
    src = torch.from_numpy(np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()).to("cuda")
    comp = gpu.Compressor(nb, 2, clevel=5, shuffle=1)
    cap = comp.max_bytes(3)
    fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(4, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), nb, 3, fr.data_ptr(), cap, off.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = off.cpu().numpy()
    f = fr.cpu().numpy()
    real = [f[o[i]:o[i + 1]].tobytes() for i in range(3)]
    comp.close()
    frames = [b"", real[0], b"", b"", real[1], real[2], b""]
    dec = gpu.Decompressor(nb, len(frames))
    got = decode_host_frames(gpu, dec, frames, nb)
    dec.close()
    want = [None, 0, None, None, 1, 2, None]
    assert got.pads_untouched
    for i, w in enumerate(want):
        if w is None:
            assert got.status[i] == SKIPPED and not got.chunks[i].any(), i
        else:
            assert got.status[i] == OK and got.chunks[i].tobytes() == chunks[w], i


@pytest.mark.parametrize("source", MUTATED)
def test_malformed_frames_are_statuses(gpu, source):
    """The named mutations (the bytes the CPU program handled cleanly under the
    sanitizers) mixed with good frames in one run: each gets its status, the
    good frames decode exactly, nothing outside the chunks is written."""
    good = {name: fr for name, fr, *_ in load_golden()}[source]
    nb = header(good)["nbytes"]
    want = oracle_decode(good)
    muts = named_mutations(good)
    assert all(cb == nb for _, _, cb, _ in muts)
    frames, expect = [good], [OK]
    for _, data, _, status in muts:
        frames += [data, good]
        expect += [status, OK]
    dec = gpu.Decompressor(nb, len(frames))
    got = decode_host_frames(gpu, dec, frames, nb)
    dec.close()
    assert got.pads_untouched
    names = ["good"] + [x for m in muts for x in (m[0], "good")]
    for i, (st, name) in enumerate(zip(expect, names)):
        assert got.status[i] == st, (name, got.status[i], st)
        if st == OK:
            assert got.chunks[i].tobytes() == want, (i, name)
    assert {BAD_HEADER, CORRUPT, UNSUPPORTED} <= set(expect)


def test_zstd_frames_are_unsupported(gpu):
    torch = _torch()
    rng = np.random.default_rng(8)
    n, n_px = 2, 20000
    nb = 2 * n_px
    src = torch.from_numpy(np.stack([camera_like(rng, n_px, np.uint16).view(np.uint8)
                                     for _ in range(n)])).to("cuda")
    dec = gpu.Decompressor(nb, n)
    for codec, shuffle in ((gpu.CODEC_BLOSC_ZSTD, 1), (gpu.CODEC_ZSTD, 0)):
        comp = gpu.Compressor(nb, 2, codec=codec, clevel=3, shuffle=shuffle)
        cap = comp.max_bytes(n)
        fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
        off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
        comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(),
                     torch.cuda.current_stream().cuda_stream)
        got = run_decoder(gpu, dec, fr, cap, off, n, nb, 16)
        comp.close()
        assert (got.status == UNSUPPORTED).all(), (codec, got.status)
        assert got.pads_untouched
    dec.close()


# ---- stage verification ----------------------------------------------------
DIMS = [(TIME, 0, 2, 1), (SPACE, 512, 128, 1), (SPACE, 384, 128, 1)]


def _frames():
    frames = synthetic_frames(U16, 6, 512, 384, 9)
    frames[:, :128, :] = 0          # one row of chunks without data: skipped
    return frames


def _literal_byte(frame: bytes) -> int:
    """Position of a byte inside the literals of the frame's first LZ4 stream
    (a payload byte of a memcpyed frame)."""
    if header(frame)["flags"] & 0x2:
        return 16 + 5
    for _, _, pos, cs, n in streams(frame):
        if cs == n:
            return pos + 4 + n // 2
        for t, ll, _, _ in lz4_sequences(frame[pos + 4:pos + 4 + cs]):
            if ll:
                return pos + 4 + t + 1 + (0 if ll < 15 else (ll - 15) // 255 + 1)
    raise AssertionError("no literal in this frame")


@pytest.mark.parametrize("shuffle", [1, 2])
def test_stage_verify_layer(gpu, shuffle):
    torch = _torch()
    frames = _frames()
    st = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    L = st.n_levels()
    lay = [st.layout(l) for l in range(L)]
    seen = set()
    damaged = False
    for b in range(0, len(frames), 2):
        st.append(np.ascontiguousarray(frames[b:b + 2]))
        for l in range(L):
            layer = st.frames_written(l) // lay[l]["frames_per_layer"] - 1
            if layer < 0 or (l, layer) in seen:
                continue
            seen.add((l, layer))
            st.compress_layer(l, layer, clevel=5, shuffle=shuffle)
            assert st.verify_layer(l, layer) == (0, UINT32_MAX), (l, layer)
            if l != 0 or damaged:
                continue
            damaged = True
            data, _ = st.copy_compressed(l, layer)
            ent = st.compressed_entries(l, layer)
            assert any(nb == 0 for *_, nb in ent), "the zero rows give skipped chunks"
            # an untouched device copy verifies
            dev = torch.from_numpy(data.copy()).to("cuda")
            assert st.verify_layer(l, layer, dev.data_ptr(), dev.numel()) == (0, UINT32_MAX)
            # one byte inside the literals of one frame
            real = [(c, o, nb) for c, _, _, o, nb in ent if nb]
            c, o, nb = real[len(real) // 2]
            bad = data.copy()
            bad[o + _literal_byte(data[o:o + nb].tobytes())] ^= 0x40
            dev = torch.from_numpy(bad).to("cuda")
            assert st.verify_layer(l, layer, dev.data_ptr(), dev.numel()) == (1, c)
            # two neighbouring frames swapped, offsets as they were
            (ca, oa, na), (cb, ob, nbb) = real[0], real[1]
            assert ob == oa + na
            sw = data.copy()
            sw[oa:oa + nbb] = data[ob:ob + nbb]
            sw[oa + nbb:oa + nbb + na] = data[oa:oa + na]
            dev = torch.from_numpy(sw).to("cuda")
            n_bad, first = st.verify_layer(l, layer, dev.data_ptr(), dev.numel())
            assert 1 <= n_bad <= 2 and first in (ca, cb), (n_bad, first)
            # and the stage's own frames still verify
            assert st.verify_layer(l, layer) == (0, UINT32_MAX)
    assert {l for l, _ in seen} == set(range(L))
    st.close()


def test_stage_verify_refusals_and_memory(gpu):
    frames = _frames()
    a = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    b = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    for st in (a, b):
        st.append(np.ascontiguousarray(frames[:2]))
    with pytest.raises(gpu.AqzError) as e:      # not compressed at all
        b.verify_layer(0, 0)
    assert e.value.status == 1
    for st in (a, b):
        st.compress_layer(0, 0, codec=gpu.CODEC_BLOSC_ZSTD, clevel=3, shuffle=1)
        st.compressed_offsets(0, 0)
    with pytest.raises(gpu.AqzError) as e:      # a zstd layer
        b.verify_layer(0, 0)
    assert e.value.status == 4
    for st in (a, b):
        st.compress_layer(0, 0, clevel=0, shuffle=1)   # lz4, stored frames
        st.compressed_offsets(0, 0)
    # nothing is allocated before the first verify
    assert a.memory_usage() == b.memory_usage()
    before = b.memory_usage()
    assert b.verify_layer(0, 0) == (0, UINT32_MAX)
    after = b.memory_usage()
    assert a.memory_usage() == before
    # the decoder state: a status and a mismatch word per chunk of the slot,
    # on the device and pinned; no copy of the layer
    words = 8 * b.layout(0)["chunks_per_layer"]
    assert after["device_bytes"] - before["device_bytes"] == words
    assert after["pinned_bytes"] - before["pinned_bytes"] == words
    with pytest.raises(gpu.AqzError) as e:      # a layer that is not resident
        b.verify_layer(0, 7)
    assert e.value.status == 1
    a.close()
    b.close()
