"""The device zstd decoder's parse on the CPU.

csrc/aqz_zstddec.hh holds the frame header and block walk, the literals and
sequences sections, the Huffman and FSE table builds, the bit readers, the
sequence decode, the repeat offsets and every bound, in one text that compiles
for host and device; the kernels of csrc/aqz_zstddec.hip add only the byte
movers.  tests/sanitize/zstddec_sanitize.cpp runs that text (and
csrc/aqz_lz4dec.hh's blosc1 container) with serial byte movers under ASan +
UBSan over a corpus written here:

  - the golden frames made by libzstd and c-blosc (tests/golden/zstd_frames.npz)
    and the valid hand-assembled frames (RLE literals, repeat offsets, ...,
    which libzstd decodes too): status OK, exact bytes;
  - frames of this library's serial encoder model (tests/zstd): OK, exact bytes;
  - split blosc-zstd frames built from per-stream libzstd output: OK, exact bytes;
  - the named mutations: exactly the expected status each;
  - 200 seeded single-byte mutations per golden frame: any status, no
    sanitizer report.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from codec_helpers import libzstd, zstd_decode
from zstddec_helpers import (GOLDEN, OK, assembled_valid, blosc_zstd_frame, byte_mutations,
                             conditions, load_golden, named_mutations, reference_decode, sha256,
                             write_corpus)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")
ZDIR = os.path.join(REPO, "tests", "zstd")

pytestmark = pytest.mark.skipif(libzstd() is None, reason="no libzstd")


def test_fixture_meets_its_conditions():
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    frames, digests = load_golden()
    conditions(frames)
    for name, (fr, n) in frames.items():
        assert sha256(reference_decode(fr, n)) == digests[name], name


def test_hand_assembled_frames_decode_with_libzstd():
    """The assembler is honest: libzstd reads every valid frame it makes, to the
    length the frame declares."""
    for name, fr, n in assembled_valid():
        assert len(zstd_decode(fr, n)) == n, name
    # spot checks of what the sequences mean
    by = {name: (fr, n) for name, fr, n in assembled_valid()}
    assert zstd_decode(*by["overlapping_match"]) == b"ab" * 101 + b"b" * 70
    assert zstd_decode(*by["rle_block"]) == b"\x5a" * 1000


def split_blosc_frames():
    """Relabelled-by-construction split blosc-zstd frames (neither c-blosc 1.21 nor
    this library splits zstd blocks)."""
    rng = np.random.default_rng(77)
    out = []
    for ts, sh, bs, n in ((2, 1, 4096, 4096 * 2 + 600), (4, 2, 8192, 8192 * 3), (8, 1, 2048, 5000),
                          (4, 0, 4096, 4096 + 4)):
        a = (rng.integers(0, 50, n // ts) + 1000).astype({2: np.uint16, 4: np.uint32,
                                                           8: np.uint64}[ts])
        data = a.tobytes() + bytes(n - a.nbytes)
        out.append((f"split_ts{ts}_sh{sh}", blosc_zstd_frame(data, ts, sh, bs, split=True), data))
    return out


def model_frames():
    """Frames of the serial model of the device encoder (tests/zstd/zstd_host.cpp),
    at the sizes test_model_frames_through_ctypes uses."""
    r = subprocess.run(["make", "-C", ZDIR], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    L = C.CDLL(os.path.join(ZDIR, "libzstd_host.so"))
    L.zh_encode_frame.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64]
    L.zh_encode_frame.restype = C.c_uint64
    rng = np.random.default_rng(3)
    out = []
    for n in (1, 777, 32768, 100003):
        for kind in range(3):
            src = {0: rng.integers(0, 256, n, dtype=np.uint8),
                   1: np.zeros(n, np.uint8),
                   2: (rng.normal(100, 4, n).clip(0, 255)).astype(np.uint8)}[kind]
            for lz in (0, 1):
                buf = np.zeros(n + 4096, np.uint8)
                k = L.zh_encode_frame(src.ctypes.data, n, lz, buf.ctypes.data, buf.size)
                assert k > 0
                out.append((f"model_n{n}_k{kind}_lz{lz}", buf[:k].tobytes(), src.tobytes()))
    return out


def corpus_records():
    records = []
    frames, digests = load_golden()
    for name, (fr, n) in frames.items():
        want = reference_decode(fr, n)
        assert sha256(want) == digests[name], name
        records.append((name, fr, n, OK, want))
    for name, fr, n in assembled_valid():
        records.append((f"assembled_{name}", fr, n, OK, zstd_decode(fr, n)))
    for name, fr, want in split_blosc_frames() + model_frames():
        records.append((name, fr, len(want), OK, want))
    for name, fr, n, status in named_mutations(frames):
        records.append((name, fr, n, status, b""))
    for i, (name, (fr, n)) in enumerate(frames.items()):
        for pos, data in byte_mutations(fr, seed=2000 + i):
            records.append((f"{name}:byte{pos}", data, n, -1, b""))
    return records


def test_decoder_parse_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "zstddec_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "sanitize", "zstddec_sanitize.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    records = corpus_records()
    corpus = str(tmp_path / "corpus.bin")
    write_corpus(corpus, records)
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, corpus], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert f"clean: {len(records)} records" in r.stdout
    assert "runtime error" not in r.stderr
    # every record with an expected status was reported with exactly it
    got = {}
    for line in r.stdout.splitlines():
        if not line.startswith(("FAIL", "clean")):
            name, st = line.rsplit(" ", 1)
            got.setdefault(name, int(st))
    for name, _, _, status, _ in records:
        if status >= 0:
            assert got[name] == status, name
    expected = {status for _, _, _, status, _ in records}
    assert {0, 2, 3, 4} <= expected
