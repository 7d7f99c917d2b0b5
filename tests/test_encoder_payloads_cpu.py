"""The encoder payload family (tests/encoder_payloads.py) before it meets a
GPU: every kind is deterministic and exact in length, the serial model of the
device zstd encoder (tests/zstd/libzstd_host.so: the format pieces of
aqz_zstd.hh) turns every kind into a frame libzstd decodes exactly, and the
normalised-count reader of zstddec_helpers (RFC 8878 4.1.1) parses every FSE
table description of the golden libzstd frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import encoder_payloads as ep
from codec_helpers import libzstd, zstd_decode
from zstddec_helpers import inspect, load_golden, read_ncount

ZDIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "zstd")
SIZES = (1, 63, 4097, 70001)


@pytest.fixture(scope="module")
def model():
    r = subprocess.run(["make", "-C", ZDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(os.path.join(ZDIR, "libzstd_host.so"))
    L.zh_encode_frame.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
    L.zh_encode_frame.restype = C.c_uint64
    return L


def test_kinds_named_by_the_family():
    assert len(ep.NAMES) == 29 and len(set(ep.NAMES)) == 29
    assert {f"period_{p}" for p in (1, 3, 4, 5, 251, 4095, 4096, 4099, 8209)} <= set(ep.NAMES)
    assert {f"tail_copy_{k}" for k in (7, 5, 4, 3)} <= set(ep.NAMES)
    assert set(ep.LZ4_NAMES) <= set(ep.NAMES)


@pytest.mark.parametrize("name", ep.NAMES)
def test_deterministic_and_exact_in_length(name):
    for n in SIZES:
        a, b = ep.make(name, n, seed=5), ep.make(name, n, seed=5)
        assert a.dtype == np.uint8 and a.shape == (n,)
        assert np.array_equal(a, b), (name, n)
    if name not in ("zeros", "const", "ramp251"):
        assert not np.array_equal(ep.make(name, 4097, seed=5), ep.make(name, 4097, seed=6))


def test_kinds_are_what_they_say():
    n = 70001
    assert not ep.make("zeros", n).any() and (ep.make("const", n) == 0xA5).all()
    for name, vals in (("two_values_50", 2), ("two_values_01", 2), ("nibble_uniform", 16),
                       ("skewed_deep", 256)):
        assert len(np.unique(ep.make(name, n))) == vals, name
    rare = np.bincount(ep.make("two_values_01", n), minlength=256)[0xEE]
    assert 0.005 * n < rare < 0.02 * n
    cnt = np.bincount(ep.make("nibble_uniform", 4096), minlength=256)
    assert set(cnt[cnt > 0]) == {256} and ep.make("nibble_uniform", n).max() < 128
    t = ep.make("text", n)
    assert t.min() >= 32 and t.max() <= 126
    for p in ep.PERIODS:
        a = ep.make(f"period_{p}", n)
        assert np.array_equal(a[p:], a[:-p]), p
    for k in ep.TAILS:
        a = ep.make(f"tail_copy_{k}", n)
        assert np.array_equal(a[n - k:], a[n - k - 64:n - 64]), k
    # the ladders: every stated run length and every stated gap, in order
    a = ep.make("run_ladder", n)
    ends = np.flatnonzero(a != 0x5A)
    runs = np.diff(np.concatenate([[-1], ends])) - 1
    want = ep.RUN_LENGTHS
    assert len(runs) >= len(want)
    # a closing byte is fresh: one in 256 equals the run's value and joins two runs
    assert sum(int(r) == w for r, w in zip(runs, want)) >= len(want) - 3
    assert {1, 40, 63, 66, 127, 131, 255, 259, 270, 275, 511, 516, 1023, 1026, 4090, 4100} <= \
        set(want)
    assert {0, 70, 127, 130, 4000, 4095, 4096, 4097, 8000} <= set(ep.LITERAL_GAPS)
    a = ep.make("literal_ladder", n).tobytes()
    pos, word = 16, a[8:16]
    for k in ep.LITERAL_GAPS:
        assert a[pos + k:pos + k + 8] == word, k
        pos += k + 8
    # raw spans: random bytes there (all 256 values), dim camera data elsewhere
    for name, s in (("raw_head", 0), ("raw_middle", n // 2 // 8192 * 8192)):
        a = ep.make(name, n)
        assert len(np.unique(a[s:s + ep.RAW_SPAN])) == 256, name
        rest = np.concatenate([a[:s], a[s + ep.RAW_SPAN:]])
        assert len(np.unique(rest)) < 64, name
    a = ep.make("short_and_long", n)
    assert np.array_equal(a[n // 2 + 4096:], a[n // 2:-4096])


@pytest.mark.skipif(libzstd() is None, reason="no libzstd")
@pytest.mark.parametrize("name", ep.NAMES)
def test_serial_model_frames_decode(model, name):
    for n in SIZES:
        src = ep.make(name, n, seed=1)
        for lz in (0, 1):
            out = np.zeros(n + 4096, np.uint8)
            k = model.zh_encode_frame(src.ctypes.data, n, lz, out.ctypes.data, out.size)
            assert k > 0, (name, n, lz)
            fr = out[:k].tobytes()
            assert zstd_decode(fr, n) == src.tobytes(), (name, n, lz)
            info = inspect(fr)
            assert info["single_segment"] and info["fcs"] == n


def test_ncount_reader_known_descriptions():
    """RFC 8878's reading, on descriptions written out by hand: accuracy log 5,
    the probabilities below."""
    def write(log, norm):
        # the RFC's writer, bit by bit (the reader's inverse, not the encoder's code)
        acc, nb = log - 5, 4
        remaining = 1 << log
        i = 0
        while i < len(norm):
            v = norm[i] + 1
            width = (remaining + 1).bit_length()
            low = (1 << width) - 1 - (remaining + 1)
            if v < low:
                acc |= v << nb
                nb += width - 1
            else:
                if v >= 1 << (width - 1):
                    v += low
                acc |= v << nb
                nb += width
            remaining -= abs(norm[i])
            i += 1
            if norm[i - 1] == 0:
                z = 0
                while i < len(norm) and norm[i] == 0:
                    z, i = z + 1, i + 1
                while z >= 3:
                    acc |= 3 << nb
                    nb, z = nb + 2, z - 3
                acc |= z << nb
                nb += 2
        assert remaining == 0
        return acc.to_bytes((nb + 7) // 8, "little")

    for log, norm in ((5, [16, 8, 4, 2, 1, 1]), (5, [30, -1, -1]), (6, [1] * 64),
                      (7, [100, 0, 0, 0, 20, 0, 8]), (9, [500] + [0] * 30 + [11, -1]),
                      (8, [-1] * 10 + [0] * 3 + [246]), (5, [31, 0, 1])):
        d = write(log, norm)
        got, glog, used = read_ncount(b"\x77" + d + b"\x00\x00", 1, 9)
        assert (got, glog, used) == (norm, log, len(d)), (norm, got, glog, used)
    with pytest.raises(AssertionError):
        read_ncount(write(9, [512]), 0, 8)


def test_ncount_reader_on_golden_libzstd_frames():
    frames, _ = load_golden()
    tables = 0
    logs = set()
    for name, (fr, _) in frames.items():
        if name.startswith("blosc_"):
            continue
        for blk in inspect(fr)["blocks"]:
            if not blk.get("modes") or "fse" not in blk["modes"]:
                continue
            for k, (mode, tab) in enumerate(zip(blk["modes"], blk["tables"])):
                assert (tab is not None) == (mode == "fse"), (name, blk["pos"], k)
                if tab is None:
                    continue
                assert sum(abs(c) for c in tab["norm"]) == 1 << tab["log"], (name, blk["pos"], k)
                assert 5 <= tab["log"] <= (9, 8, 9)[k]
                assert len(tab["norm"]) <= (36, 32, 53)[k]
                assert tab["minus1"] == (-1 in tab["norm"])
                tables += 1
                logs.add(tab["log"])
            if blk["modes"] == ("fse",) * 3:
                assert blk["table_logs"] == tuple(t["log"] for t in blk["tables"])
            # the bitstream follows the descriptions inside the block
            assert blk["tables_end"] < blk["pos"] + 3 + blk["size"]
    assert tables >= 10 and len(logs) >= 2


def _stored_blosc_frame(data: bytes, ts: int, shuffle: int, blocksize: int) -> bytes:
    """A blosc1 frame (LZ4 codec id, unsplit blocks) whose blocks are shuffled
    by the oracle and stored as they are (csize = block bytes)."""
    import struct
    from codec_helpers import shuffle as shuf
    n = len(data)
    nblocks = -(-n // blocksize)
    flags = (1 << 5) | 0x10 | (1 if shuffle == 1 else 4)
    base = 16 + 4 * nblocks
    body, starts = b"", []
    for j in range(nblocks):
        blk = data[j * blocksize:(j + 1) * blocksize]
        blk = shuf("shuffle" if shuffle == 1 else "bitshuffle", ts, blk)
        starts.append(base + len(body))
        body += struct.pack("<I", len(blk)) + blk
    return (bytes([2, 1, flags, ts]) + struct.pack("<III", n, blocksize, base + len(body)) +
            struct.pack("<%dI" % nblocks, *starts) + body)


@pytest.mark.parametrize("shuffle", [1, 2])
def test_shuffled_block_with_bytes_after_its_last_element(shuffle):
    """A last block that is no whole number of elements (a chunk of 70001 bytes at
    typesize 2 in blocks of 8192): c-blosc's decoder un-shuffles its whole
    elements -- bit-wise when they are a multiple of 8 -- and copies the bytes
    after them, so that is what the oracle's shuffles (the device encoder's
    yardstick) must do.  (Regression: the bitshuffle left such a block
    unshuffled, and c-blosc decoded device frames of it to other bytes.)"""
    from codec_helpers import libblosc, libblosc_decode, oracle_decode, shuffle as shuf
    rng = np.random.default_rng(12)
    for ts, bs, n in ((2, 8192, 70001), (4, 64, 2 * 64 + 35), (8, 1024, 1024 + 67),
                      (2, 16, 16 + 5), (4, 4096, 4096 + 3)):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        fr = _stored_blosc_frame(data, ts, shuffle, bs)
        assert oracle_decode(fr) == data, (ts, bs, n)
        if libblosc() is not None:
            assert libblosc_decode(fr) == data, (ts, bs, n)
        last = data[n // bs * bs:]
        kind = "shuffle" if shuffle == 1 else "bitshuffle"
        sh = shuf(kind, ts, last)
        ne = len(last) // ts
        assert sh[ne * ts:] == last[ne * ts:]
        whole = shuffle == 1 or ne % 8 == 0
        assert (sh[:ne * ts] == shuf(kind, ts, last[:ne * ts])) and \
            ((sh != last) == (whole and ne > 1)), (ts, bs, n)
