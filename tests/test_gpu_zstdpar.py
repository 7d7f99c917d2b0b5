"""GPU tests of the block-parallel zstd decode (AQZ_DECODE_ZSTD_PARALLEL,
csrc/aqz_zstdpar.hip).  Every decoder here is created with
DECODE_CODEC_ZSTD | DECODE_ZSTD_PARALLEL: frames of the device encoder, of
libzstd (tests/golden/zstd_frames.npz) and of the hand-assembler decode to
exactly the chunk bytes, malformed frames get the serial decoder's statuses,
compare mode and the reader work through it, and last_run_counts() shows that
the parallel kernels, not the serial fallback, produced the bytes."""
import numpy as np
import pytest

from codec_helpers import camera_like, chunk_payloads, libzstd, zstd_decode
from decoder_helpers import byte_mutations
from oracle_bindings import MEAN, SPACE, TIME, U16, synthetic_frames
from test_gpu_decode import decode_host_frames, run_decoder
from test_gpu_zstddec import _good_frame, compress_on_device, host_frames
from zstddec_helpers import (BAD_HEADER, CORRUPT, OK, SKIPPED, UNSUPPORTED, assembled_valid,
                             inspect, load_golden, named_mutations, reference_decode, sha256)
from zstdpar_helpers import assembled_parallel, over_capacity_frame

pytestmark = pytest.mark.gpu

UINT32_MAX = (1 << 32) - 1
MAGIC = b"\x28\xb5\x2f\xfd"


def _codecs(gpu):
    return gpu.DECODE_CODEC_ZSTD | gpu.DECODE_ZSTD_PARALLEL


def _decoder(gpu, max_chunk_bytes, max_chunks):
    dec = gpu.Decompressor(max_chunk_bytes, max_chunks, codecs=_codecs(gpu))
    assert dec.scratch_bytes() == gpu.decompressor_scratch_bytes(max_chunk_bytes, max_chunks,
                                                                _codecs(gpu))
    return dec


def _is_plain(fr):
    return bytes(fr[:4]) == MAGIC


def _compressed_blocks(frames):
    return sum(1 for fr in frames for b in inspect(fr)["blocks"] if b["type"] == "compressed")


def _sequences(frames):
    return sum(b.get("nseq", 0) for fr in frames for b in inspect(fr)["blocks"])


def round_trip(gpu, chunks, clevel, pad):
    n, nb = chunks.shape
    fr, cap, off = compress_on_device(gpu, chunks, 2, gpu.CODEC_ZSTD, clevel, 0)
    dec = _decoder(gpu, nb, n)
    got = run_decoder(gpu, dec, fr, cap, off, n, nb, pad)
    counts = dec.last_run_counts()
    dec.close()
    what = (clevel, nb)
    assert (got.status == OK).all(), (what, got.status)
    assert np.array_equal(got.chunks, chunks), what
    assert got.pads_untouched, what
    host = host_frames(fr, off)
    assert all(_is_plain(f) for f in host)
    assert counts["parallel_frames"] == n and counts["serial_frames"] == 0, (what, counts)
    assert counts["blocks"] == _compressed_blocks(host), (what, counts)
    assert counts["sequences"] == _sequences(host), (what, counts)


@pytest.mark.parametrize("level", [1, 3, 9])
def test_round_trip_device_encoder(gpu, level):
    rng = np.random.default_rng(200 + level)
    for n_px, pad in ((50, 3), (1000, 0), (16384, 40), (100_003 // 2, 17)):
        pay = chunk_payloads(rng, np.uint16, n_px)
        chunks = np.stack([a.view(np.uint8) for a in pay.values()])
        round_trip(gpu, chunks, level, pad)


def test_round_trip_far_matches(gpu):
    """The repeated plane of test_gpu_zstddec: 74 blocks, matches across many."""
    rng = np.random.default_rng(5)
    plane = camera_like(rng, 100_000, np.uint16).view(np.uint8)
    chunk = np.concatenate([plane, plane, plane])
    assert chunk.size == 600_000
    round_trip(gpu, chunk[None, :], 9, pad=9)


def test_golden_libzstd_frames(gpu):
    frames, digests = load_golden()
    groups = {}
    for name, (fr, n) in frames.items():
        if n:
            groups.setdefault(n, []).append((name, fr))
    dec = _decoder(gpu, max(groups), max(len(g) for g in groups.values()))
    for n, items in sorted(groups.items()):
        got = decode_host_frames(gpu, dec, [fr for _, fr in items], n, pad=7)
        counts = dec.last_run_counts()
        assert got.pads_untouched, n
        for i, (name, fr) in enumerate(items):
            assert got.status[i] == OK, (name, got.status[i])
            data = got.chunks[i].tobytes()
            assert sha256(data) == digests[name], name
            assert data == reference_decode(fr, n), name
        plain = [fr for _, fr in items if _is_plain(fr)]
        # blosc1-zstd frames stay on the serial kernel
        assert counts["parallel_frames"] == len(plain), (n, counts)
        assert counts["serial_frames"] == len(items) - len(plain), (n, counts)
        assert counts["blocks"] == _compressed_blocks(plain), (n, counts)
    dec.close()


@pytest.mark.skipif(libzstd() is None, reason="no libzstd")
def test_assembled_frames(gpu):
    """The hand-assembled frames of the serial decoder's tests and the ones aimed at
    the phases (record batches of 63 / 64 / 65 / 129, all-dependent and independent
    batches, repeat codes at block starts, table definers two blocks back), against
    libzstd's bytes; the frame with more blocks than the table falls back."""
    items = [(name, fr, n, True) for name, fr, n in assembled_valid() + assembled_parallel()]
    items.append(over_capacity_frame() + (False,))
    dec = _decoder(gpu, max(n for _, _, n, _ in items), 1)
    for name, fr, n, parallel in items:
        want = zstd_decode(fr, n)
        got = decode_host_frames(gpu, dec, [fr], n, pad=5)
        counts = dec.last_run_counts()
        assert got.status[0] == OK, (name, got.status)
        assert got.chunks[0].tobytes() == want, name
        assert got.pads_untouched, name
        assert (counts["parallel_frames"], counts["serial_frames"]) == \
            ((1, 0) if parallel else (0, 1)), (name, counts)
        if parallel:
            assert counts["sequences"] == _sequences([fr]), (name, counts)
    dec.close()


def test_malformed_frames_are_statuses(gpu):
    """The named mutations, each between two good frames in one run."""
    frames, _ = load_golden()
    groups = {}
    for name, data, n, status in named_mutations(frames):
        groups.setdefault(n, []).append((name, data, status))
    seen = set()
    for n, items in sorted(groups.items()):
        good, want = _good_frame(n)
        run = [good]
        for _, data, _ in items:
            run += [data, good]
        dec = _decoder(gpu, max(n, 1), len(run))
        got = decode_host_frames(gpu, dec, run, n, pad=11)
        dec.close()
        assert got.pads_untouched, n
        for i in range(0, len(run), 2):
            assert got.status[i] == OK and got.chunks[i].tobytes() == want, (n, i)
        for k, (name, _, status) in enumerate(items):
            assert got.status[2 * k + 1] == status, (name, got.status[2 * k + 1], status)
            seen.add(status)
    assert {BAD_HEADER, CORRUPT, UNSUPPORTED} <= seen


def test_byte_mutations_match_the_serial_decoder(gpu):
    """One seeded set of single-byte mutations of text_windowed, in one run of each
    decoder: the same status, and the same bytes where it is OK."""
    frames, _ = load_golden()
    fr, n = frames["text_windowed"]
    run = [data for _, data in byte_mutations(fr, seed=4242)]
    ser = gpu.Decompressor(n, len(run), codecs=gpu.DECODE_CODEC_ZSTD)
    want = decode_host_frames(gpu, ser, run, n, pad=3)
    ser.close()
    dec = _decoder(gpu, n, len(run))
    got = decode_host_frames(gpu, dec, run, n, pad=3)
    counts = dec.last_run_counts()
    dec.close()
    assert got.pads_untouched
    assert np.array_equal(got.status, want.status), np.flatnonzero(got.status != want.status)
    ok = got.status == OK
    assert np.array_equal(got.chunks[ok], want.chunks[ok])
    assert counts["parallel_frames"] + counts["serial_frames"] == len(run)
    # a damaged block header can make the walk see many more blocks: those few fall back
    assert counts["parallel_frames"] >= len(run) - 10, counts


def test_mixed_run(gpu):
    """Plain zstd, blosc-zstd, LZ4 and zero-length frames in one run: the plain
    frames take the parallel path, blosc-zstd the serial kernel, and an LZ4 frame is
    not this decoder's."""
    rng = np.random.default_rng(9)
    n_px = 20_000
    nb = 2 * n_px
    chunk = camera_like(rng, n_px, np.uint16).view(np.uint8)[None, :]
    lz4 = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_BLOSC_LZ4, 5, 1)[::2])[0]
    bz = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_BLOSC_ZSTD, 3, 2)[::2])[0]
    pz = host_frames(*compress_on_device(gpu, chunk, 2, gpu.CODEC_ZSTD, 5, 0)[::2])[0]
    run = [pz, b"", lz4, bz, pz, b"", bz, pz]
    kind = ["p", "s", "l", "b", "p", "s", "b", "p"]
    dec = _decoder(gpu, nb, len(run))
    got = decode_host_frames(gpu, dec, run, nb, pad=13)
    counts = dec.last_run_counts()
    dec.close()
    assert got.pads_untouched
    for i, k in enumerate(kind):
        if k == "s":
            assert got.status[i] == SKIPPED and not got.chunks[i].any(), i
        elif k == "l":
            assert got.status[i] == UNSUPPORTED, (i, got.status)
        else:
            assert got.status[i] == OK, (i, got.status)
            assert np.array_equal(got.chunks[i], chunk[0]), i
    assert counts["parallel_frames"] == 3 and counts["serial_frames"] == 2, counts
    assert counts["blocks"] == _compressed_blocks([pz]) * 3, counts
    # the option bit alone, or next to the LZ4 family, is refused
    for codecs in (gpu.DECODE_ZSTD_PARALLEL, gpu.DECODE_ZSTD_PARALLEL | gpu.DECODE_CODEC_LZ4):
        with pytest.raises(gpu.AqzError) as e:
            gpu.Decompressor(nb, 1, codecs=codecs)
        assert e.value.status == 1


# ---- compare mode through a stage, and the reader ------------------------------------
DIMS = [(TIME, 0, 2, 1), (SPACE, 512, 128, 1), (SPACE, 384, 128, 1)]


def test_stage_verify_with_the_flag(gpu, monkeypatch):
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    import torch
    frames = synthetic_frames(U16, 2, 512, 384, 9)
    st = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    lay = [st.layout(l) for l in range(st.n_levels())]
    with pytest.raises(gpu.AqzError) as e:
        st.verify_prepare(gpu.DECODE_ZSTD_PARALLEL)
    assert e.value.status == 1
    before = st.memory_usage()
    st.verify_prepare(_codecs(gpu))
    prepared = st.memory_usage()
    device = 0
    for L in lay:
        n, nb = L["chunks_per_layer"], L["bytes_per_chunk"]
        device += gpu.decompressor_scratch_bytes(nb, n, _codecs(gpu))
        device += L["layer_slots"] * 8 * n + 8 * (n + 1)
    assert prepared["device_bytes"] - before["device_bytes"] == device
    st.append(np.ascontiguousarray(frames))
    st.compress_layer(0, 0, codec=gpu.CODEC_ZSTD, clevel=3, shuffle=0)
    with_comp = st.memory_usage()
    assert st.verify_layer(0, 0) == (0, UINT32_MAX)
    assert st.memory_usage() == with_comp
    data, _ = st.copy_compressed(0, 0)
    ent = st.compressed_entries(0, 0)
    real = [(c, o, nb) for c, _, _, o, nb in ent if nb]
    c, o, nb = real[len(real) // 2]
    bad = data.copy()
    bad[o + nb // 2] ^= 0x40
    dev = torch.from_numpy(bad).to("cuda")
    assert st.verify_layer(0, 0, dev.data_ptr(), dev.numel()) == (1, c)
    assert st.verify_layer(0, 0) == (0, UINT32_MAX)
    st.close()


def test_reader_with_the_flag(gpu, monkeypatch):
    """A reader created with the flag hands back the appended frames of a zstd
    layer bit for bit."""
    monkeypatch.setenv("AQZ_ZSTD_HOST", "0")
    import torch
    from test_gpu_reader import as_bytes, read_back
    frames = synthetic_frames(U16, 2, 512, 384, 11)
    st = gpu.Stage(DIMS, U16, MEAN, layer_slots=2, max_batch_frames=2)
    rd = gpu.Reader(st.level_dims(0), U16, codecs=_codecs(gpu))
    assert rd.device_bytes() == gpu.reader_device_bytes(st.level_dims(0), U16,
                                                        codecs=_codecs(gpu)) > 0
    st.append(np.ascontiguousarray(frames))
    st.compress_layer(0, 0, codec=gpu.CODEC_ZSTD, clevel=3, shuffle=0)
    off = st.compressed_offsets(0, 0)
    total = int(off[-1])
    dev = torch.empty(max(total, 1), dtype=torch.uint8, device="cuda")
    st.copy_compressed_async(0, 0, dev.data_ptr(), total)
    st.wait_copies()
    rd.load_frames(dev, off, None, gpu.CODEC_ZSTD, frames_bytes=total,
                   stream_ptr=torch.cuda.current_stream().cuda_stream)
    got = read_back(rd, 0, rd.layout()["frames_per_layer"])
    status, bad = rd.status()
    assert bad == 0 and (status == OK).all(), status
    assert np.array_equal(got, as_bytes(frames))
    rd.close()
    st.close()
