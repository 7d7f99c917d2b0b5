"""GPU tests of the device zstd decoder (aqz_decompressor_create_for with
AQZ_DECODE_CODEC_ZSTD) and of the stage's on-device verification of zstd layers
(aqz_stage_verify_prepare): frames made by the device compressor, by libzstd and
c-blosc themselves (tests/golden/zstd_frames.npz) and by the hand-assembler
(repeat offsets, RLE literals) decode on the device to exactly the chunk bytes,
bytes outside the chunks stay untouched, malformed frames get their status and
leave their neighbours alone, frames of every kind mix in one run, and a stage
verifies its own zstd layers and reports a damaged copy of them."""
import numpy as np
import pytest

from codec_helpers import camera_like, chunk_payloads, libzstd, zstd_compress
from oracle_bindings import MEAN, SPACE, TIME, U16, synthetic_frames
from test_gpu_decode import FILL, decode_host_frames, run_decoder  # noqa: F401
from zstddec_helpers import (BAD_HEADER, CORRUPT, OK, SKIPPED, UNSUPPORTED, assemble_frame,
                             assembled_valid, blosc_zstd_frame, load_golden, named_mutations,
                             reference_decode, sha256)

pytestmark = pytest.mark.gpu

DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
UINT32_MAX = (1 << 32) - 1


def _torch():
    import torch
    return torch


def compress_on_device(gpu, chunks: np.ndarray, ts, codec, clevel, shuffle):
    """(frames tensor, capacity, offsets tensor) of the device compressor."""
    torch = _torch()
    n, nb = chunks.shape
    src = torch.from_numpy(np.ascontiguousarray(chunks)).to("cuda")
    comp = gpu.Compressor(nb, ts, codec=codec, clevel=clevel, shuffle=shuffle)
    cap = comp.max_bytes(n)
    fr = torch.empty(cap, dtype=torch.uint8, device="cuda")
    off = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    comp.run_ptr(src.data_ptr(), nb, n, fr.data_ptr(), cap, off.data_ptr(),
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    comp.close()
    return fr, cap, off


def host_frames(fr, off):
    o = off.cpu().numpy()
    f = fr.cpu().numpy()
    return [f[o[i]:o[i + 1]].tobytes() for i in range(len(o) - 1)]


def round_trip(gpu, chunks: np.ndarray, ts, codec, clevel, shuffle, pad):
    """Compressor then Decompressor, the frames never leaving the device."""
    n, nb = chunks.shape
    fr, cap, off = compress_on_device(gpu, chunks, ts, codec, clevel, shuffle)
    dec = gpu.Decompressor(nb, n, codecs=gpu.DECODE_CODEC_ZSTD)
    got = run_decoder(gpu, dec, fr, cap, off, n, nb, pad)
    dec.close()
    what = (codec, ts, clevel, shuffle, nb)
    assert (got.status == OK).all(), (what, got.status)
    assert np.array_equal(got.chunks, chunks), what
    assert got.pads_untouched, what


@pytest.mark.parametrize("ts", [1, 2, 4, 8])
@pytest.mark.parametrize("shuffle", [0, 1, 2])
def test_round_trip_blosc_zstd(gpu, ts, shuffle):
    rng = np.random.default_rng(100 + 10 * ts + shuffle)
    for n_px, pad in ((50, 3), (1000, 0), (16384, 40), (100_003 // ts, 17)):
        pay = chunk_payloads(rng, DT[ts], n_px)
        chunks = np.stack([a.view(np.uint8) for a in pay.values()])
        round_trip(gpu, chunks, ts, gpu.CODEC_BLOSC_ZSTD, 3, shuffle, pad)


@pytest.mark.parametrize("level", [1, 3, 5, 9])
def test_round_trip_plain_zstd(gpu, level):
    rng = np.random.default_rng(200 + level)
    for n_px, pad in ((50, 3), (1000, 0), (16384, 40), (100_003 // 2, 17)):
        pay = chunk_payloads(rng, np.uint16, n_px)
        chunks = np.stack([a.view(np.uint8) for a in pay.values()])
        round_trip(gpu, chunks, 2, gpu.CODEC_ZSTD, level, 0, pad)


def test_round_trip_far_matches(gpu):
    """A repeated plane: matches reach back farther than 160 KiB, across many of
    the encoder's 8 KiB blocks."""
    rng = np.random.default_rng(5)
    plane = camera_like(rng, 100_000, np.uint16).view(np.uint8)
    chunk = np.concatenate([plane, plane, plane])
    assert chunk.size == 600_000
    round_trip(gpu, chunk[None, :], 2, gpu.CODEC_ZSTD, 9, 0, pad=9)


def _good_frame(n):
    """A valid plain frame of n bytes (raw blocks) and its payload."""
    data = (np.arange(n) % 253).astype(np.uint8).tobytes()
    blocks = [("raw", data[i:i + 100_000]) for i in range(0, n, 100_000)] or [("raw", b"")]
    return assemble_frame(blocks), data


def test_golden_libzstd_and_cblosc_frames(gpu):
    """Every frame libzstd / c-blosc made decodes to its payload: the sha256
    recorded with it and the host reference's decode.  One run per chunk size."""
    frames, digests = load_golden()
    groups = {}
    for name, (fr, n) in frames.items():
        if n:
            groups.setdefault(n, []).append((name, fr))
    dec = gpu.Decompressor(max(groups), max(len(g) for g in groups.values()),
                           codecs=gpu.DECODE_CODEC_ZSTD)
    for n, items in sorted(groups.items()):
        got = decode_host_frames(gpu, dec, [fr for _, fr in items], n, pad=7)
        assert got.pads_untouched, n
        for i, (name, fr) in enumerate(items):
            assert got.status[i] == OK, (name, got.status[i])
            data = got.chunks[i].tobytes()
            assert sha256(data) == digests[name], name
            assert data == reference_decode(fr, n), name
    dec.close()


@pytest.mark.skipif(libzstd() is None, reason="no libzstd")
def test_hand_assembled_and_split_frames(gpu):
    """Repeat-offset codes, RLE literals, matches across blocks (frames libzstd
    does not emit on request; it decodes them: the expected bytes), and blosc-zstd
    frames whose blocks are split into typesize streams."""
    from codec_helpers import zstd_decode
    items = [(name, fr, zstd_decode(fr, n)) for name, fr, n in assembled_valid()]
    rng = np.random.default_rng(77)
    for ts, sh, bs, n in ((2, 1, 4096, 4096 * 2 + 600), (4, 2, 8192, 8192 * 3),
                          (8, 1, 65536, 65536 + 4000)):
        a = (rng.integers(0, 50, n // ts) + 1000).astype(DT[ts])
        data = a.tobytes() + bytes(n - a.nbytes)
        items.append((f"split_ts{ts}_sh{sh}", blosc_zstd_frame(data, ts, sh, bs, True), data))
    dec = gpu.Decompressor(max(len(w) for _, _, w in items), 1, codecs=gpu.DECODE_CODEC_ZSTD)
    for name, fr, want in items:
        got = decode_host_frames(gpu, dec, [fr], len(want), pad=5)
        assert got.status[0] == OK, (name, got.status)
        assert got.chunks[0].tobytes() == want, name
        assert got.pads_untouched, name
    dec.close()


def test_malformed_frames_are_statuses(gpu):
    """The named mutations (the bytes the CPU program handled cleanly under the
    sanitizers), each between two good frames of the same length in one run: the
    mutation gets exactly its status, the good frames decode exactly, nothing
    outside the chunks is written."""
    frames, _ = load_golden()
    muts = named_mutations(frames)
    groups = {}
    for name, data, n, status in muts:
        groups.setdefault(n, []).append((name, data, status))
    seen = set()
    for n, items in sorted(groups.items()):
        good, want = _good_frame(n)
        run = [good]
        for _, data, _ in items:
            run += [data, good]
        dec = gpu.Decompressor(max(n, 1), len(run), codecs=gpu.DECODE_CODEC_ZSTD)
        got = decode_host_frames(gpu, dec, run, n, pad=11)
        dec.close()
        assert got.pads_untouched, n
        for i in range(0, len(run), 2):
            assert got.status[i] == OK and got.chunks[i].tobytes() == want, (n, i)
        for k, (name, _, status) in enumerate(items):
            assert got.status[2 * k + 1] == status, (name, got.status[2 * k + 1], status)
            seen.add(status)
    assert {BAD_HEADER, CORRUPT, UNSUPPORTED} <= seen


def test_mixed_run_and_codec_masks(gpu):
    """blosc-lz4, memcpyed, blosc-zstd, plain zstd and zero-length frames in one
    run; a frame of a codec the decoder was not created for is UNSUPPORTED."""
    rng = np.random.default_rng(9)
    n_px = 20_000
    nb = 2 * n_px
    chunk = camera_like(rng, n_px, np.uint16).view(np.uint8)[None, :]
    noise = rng.integers(0, 256, nb, dtype=np.uint8)[None, :]
    lz4 = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_BLOSC_LZ4, 5, 1)[::2])[0]
    lz4_stored = host_frames(*compress_on_device(gpu, noise, 2, gpu.CODEC_BLOSC_LZ4, 0, 0)[::2])[0]
    bz = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_BLOSC_ZSTD, 3, 2)[::2])[0]
    pz = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_ZSTD, 5, 0)[::2])[0]
    assert (lz4[2] >> 5, bz[2] >> 5, pz[:4]) == (1, 4, b"\x28\xb5\x2f\xfd")
    run = [pz, b"", lz4, bz, lz4_stored, pz, b"", bz, lz4]
    want = [chunk, None, chunk, chunk, noise, chunk, None, chunk, chunk]
    kind = ["z", "s", "l", "z", "l", "z", "s", "z", "l"]
    for codecs in (gpu.DECODE_CODEC_LZ4 | gpu.DECODE_CODEC_ZSTD, gpu.DECODE_CODEC_ZSTD,
                   gpu.DECODE_CODEC_LZ4):
        dec = gpu.Decompressor(nb, len(run), codecs=codecs)
        assert dec.scratch_bytes() == gpu.decompressor_scratch_bytes(nb, len(run), codecs)
        got = decode_host_frames(gpu, dec, run, nb, pad=13)
        dec.close()
        assert got.pads_untouched
        for i, (w, k) in enumerate(zip(want, kind)):
            if k == "s":
                assert got.status[i] == SKIPPED and not got.chunks[i].any(), (codecs, i)
            elif (k == "z" and codecs & gpu.DECODE_CODEC_ZSTD) or \
                    (k == "l" and codecs & gpu.DECODE_CODEC_LZ4):
                assert got.status[i] == OK, (codecs, i, got.status)
                assert np.array_equal(got.chunks[i], w[0]), (codecs, i)
            else:
                assert got.status[i] == UNSUPPORTED, (codecs, i, got.status)
    # the scratch a zstd decoder documents: a slot per chunk and the literal slots
    pitch = (nb + 15) // 16 * 16
    passes = min(8, -(-nb // 32768))
    assert gpu.decompressor_scratch_bytes(nb, 9, gpu.DECODE_CODEC_ZSTD) == \
        9 * (pitch + passes * min(pitch, 128 * 1024))
    assert gpu.decompressor_scratch_bytes(nb, 9, gpu.DECODE_CODEC_LZ4) == \
        gpu.decompressor_scratch_bytes(nb, 9) == 9 * pitch
    for codecs in (0, 4, 7):
        with pytest.raises(gpu.AqzError) as e:
            gpu.Decompressor(nb, 1, codecs=codecs)
        assert e.value.status == 1
        assert gpu.decompressor_scratch_bytes(nb, 1, codecs) == 0


# ---- stage verification -------------------------------------------------------------
DIMS = [(TIME, 0, 2, 1), (SPACE, 512, 128, 1), (SPACE, 384, 128, 1)]


def _frames():
    frames = synthetic_frames(U16, 6, 512, 384, 9)
    frames[:, :128, :] = 0          # one row of chunks without data: skipped
    return frames


@pytest.mark.parametrize("codec,shuffle", [("blosc", 1), ("blosc", 2), ("blosc", 0), ("zstd", 0)])
def test_stage_verify_zstd_layers(gpu, codec, shuffle, monkeypatch):
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    torch = _torch()
    codec = gpu.CODEC_BLOSC_ZSTD if codec == "blosc" else gpu.CODEC_ZSTD
    frames = _frames()
    st = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    L = st.n_levels()
    lay = [st.layout(l) for l in range(L)]
    # what verify_prepare allocates, at the call
    before = st.memory_usage()
    with pytest.raises(gpu.AqzError) as e:
        st.verify_prepare(0)
    assert e.value.status == 1
    st.verify_prepare(gpu.DECODE_CODEC_ZSTD)
    prepared = st.memory_usage()
    device = pinned = 0
    for l in range(L):
        n, nb = lay[l]["chunks_per_layer"], lay[l]["bytes_per_chunk"]
        device += gpu.decompressor_scratch_bytes(nb, n, gpu.DECODE_CODEC_ZSTD)
        slots = lay[l]["layer_slots"]
        device += slots * 8 * n + 8 * (n + 1)   # two words per chunk and slot, offsets copy
        pinned += slots * 8 * n
    assert prepared["device_bytes"] - before["device_bytes"] == device
    assert prepared["pinned_bytes"] - before["pinned_bytes"] == pinned
    seen = set()
    damaged = False
    for b in range(0, len(frames), 2):
        st.append(np.ascontiguousarray(frames[b:b + 2]))
        for l in range(L):
            layer = st.frames_written(l) // lay[l]["frames_per_layer"] - 1
            if layer < 0 or (l, layer) in seen:
                continue
            seen.add((l, layer))
            st.compress_layer(l, layer, codec=codec, clevel=3, shuffle=shuffle)
            with_comp = st.memory_usage()
            assert st.verify_layer(l, layer) == (0, UINT32_MAX), (l, layer)
            assert st.memory_usage() == with_comp       # nothing allocated by a verify
            if l != 0 or damaged:
                continue
            damaged = True
            data, _ = st.copy_compressed(l, layer)
            ent = st.compressed_entries(l, layer)
            assert any(nb == 0 for *_, nb in ent), "the zero rows give skipped chunks"
            dev = torch.from_numpy(data.copy()).to("cuda")
            assert st.verify_layer(l, layer, dev.data_ptr(), dev.numel()) == (0, UINT32_MAX)
            # one byte in the middle of one frame
            real = [(c, o, nb) for c, _, _, o, nb in ent if nb]
            c, o, nb = real[len(real) // 2]
            bad = data.copy()
            bad[o + nb // 2] ^= 0x40
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
            # an LZ4 layer of the same stage verifies as before
            st.compress_layer(l, layer, clevel=5, shuffle=1)
            assert st.verify_layer(l, layer) == (0, UINT32_MAX)
    assert {l for l, _ in seen} == set(range(L))
    st.close()


@pytest.mark.parametrize("codec,shuffle", [("blosc", 1), ("zstd", 0)])
def test_stage_verify_host_made_layers(gpu, codec, shuffle, monkeypatch):
    """A layer whose frames the host made (AQZ_ZSTD_HOST=1: libzstd's own frames)
    has no device frames: it is refused unless a device copy is given, and the
    copy verifies against the resident chunks."""
    monkeypatch.setenv("AQZ_ZSTD_HOST", "1")
    torch = _torch()
    codec = gpu.CODEC_BLOSC_ZSTD if codec == "blosc" else gpu.CODEC_ZSTD
    frames = _frames()
    st = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    st.verify_prepare(gpu.DECODE_CODEC_ZSTD)
    st.append(np.ascontiguousarray(frames[:2]))
    st.compress_layer(0, 0, codec=codec, clevel=3, shuffle=shuffle)
    data, _ = st.copy_compressed(0, 0)
    ent = st.compressed_entries(0, 0)
    with pytest.raises(gpu.AqzError) as e:
        st.verify_layer(0, 0)
    assert e.value.status == 1
    dev = torch.from_numpy(data.copy()).to("cuda")
    assert st.verify_layer(0, 0, dev.data_ptr(), dev.numel()) == (0, UINT32_MAX)
    real = [(c, o, nb) for c, _, _, o, nb in ent if nb]
    c, o, nb = real[len(real) // 2]
    bad = data.copy()
    bad[o + nb // 2] ^= 0x40
    dev = torch.from_numpy(bad).to("cuda")
    assert st.verify_layer(0, 0, dev.data_ptr(), dev.numel()) == (1, c)
    st.close()
