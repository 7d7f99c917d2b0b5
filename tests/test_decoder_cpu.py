"""The blosc1-LZ4 decoder's parse on the CPU.

csrc/aqz_lz4dec.hh holds the header and block-start checks, the stream chain,
the LZ4 token walk with all its bounds and the un-shuffle byte map, in one text
that compiles for host and device; the kernels of csrc/aqz_decode.hip add only
the byte movers.  tests/sanitize/lz4dec_sanitize.cpp runs that text with a
serial byte mover under ASan + UBSan over a corpus written here:

  - the golden frames made by c-blosc 1.21 (tests/golden/cblosc_lz4_frames.npz):
    status OK, the payload's sha256, the oracle's decode;
  - named mutations of golden frames: exactly the expected status each;
  - 200 seeded single-byte mutations per golden frame: any status, no
    sanitizer report.
"""
import os
import subprocess

from codec_helpers import header, oracle_decode
from decoder_helpers import (GOLDEN, MUTATED, OK, byte_mutations, load_golden,
                             named_mutations, props, sha256, write_corpus)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")


def test_fixture_meets_its_conditions():
    assert os.path.getsize(GOLDEN) <= 256 * 1024
    g = load_golden()
    ps = [props(fr) for _, fr, _, _, _ in g]
    assert {ts for _, _, ts, _, _ in g} >= {1, 2, 4, 8}
    assert {sh for _, _, _, sh, _ in g} >= {0, 1, 2}
    assert any(p["memcpyed"] for p in ps)                                   # flag 0x2
    assert any(p["dont_split"] for p in ps)                                 # flag 0x10
    assert any(p["split_full_blocks"] >= 2 and p["leftover"] for p in ps)
    assert any(p["raw_stream"] and not p["memcpyed"] for p in ps)
    assert any(p["max_stream"] > 65536 for p in ps)
    for name, fr, ts, sh, digest in g:
        h = header(fr)
        assert h["version"] == 2 and h["typesize"] == ts and (h["flags"] >> 5) == 1, name
        assert h["cbytes"] == len(fr), name
        if not h["flags"] & 0x2:
            assert bool(h["flags"] & 0x1) == (sh == 1), name
            assert bool(h["flags"] & 0x4) == (sh == 2), name
        assert sha256(oracle_decode(fr)) == digest, name


def corpus_records():
    records = []
    g = load_golden()
    for name, fr, _, _, digest in g:
        want = oracle_decode(fr)
        assert sha256(want) == digest, name
        records.append((name, fr, len(want), OK, want))
    by_name = {name: fr for name, fr, *_ in g}
    for src in MUTATED:
        for mname, data, chunk_bytes, status in named_mutations(by_name[src]):
            records.append((f"{src}:{mname}", data, chunk_bytes, status, b""))
    for i, (name, fr, *_) in enumerate(g):
        nbytes = header(fr)["nbytes"]
        for pos, data in byte_mutations(fr, seed=1000 + i):
            records.append((f"{name}:byte{pos}", data, nbytes, -1, b""))
    return records


def test_decoder_parse_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "lz4dec_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "sanitize", "lz4dec_sanitize.cpp"),
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
    # every named mutation was reported with the status it must get
    got = dict(line.rsplit(" ", 1) for line in r.stdout.splitlines()
               if ":" in line and not line.startswith(("FAIL", "clean")))
    for name, _, _, status, _ in records:
        if status >= 0 and ":" in name:
            assert int(got[name]) == status, name
