"""The block-parallel zstd decode (AQZ_DECODE_ZSTD_PARALLEL) on the CPU.

csrc/aqz_zstdpar.hh holds the four phases -- index, block entropy decode,
placement, execute -- in one text for host and device, on top of
csrc/aqz_zstddec.hh's parse.  tests/sanitize/zstdpar_sanitize.cpp runs them
with serial movers over heap buffers of exactly the declared sizes under ASan +
UBSan, in the kernels' order, and runs the serial parse on the same bytes:

  - over test_zstddec_cpu.corpus_records() (golden, assembled, model and split
    blosc frames, the named mutations, 200 seeded byte mutations per golden
    frame) and the frames of zstdpar_helpers aimed at the phases;
  - every named record gets its exact status; every record the serial parse's
    status, and its bytes when OK (the program fails otherwise);
  - of the valid plain-zstd records only the one built to exceed the block
    table reports "fallback";
  - the scratch formula of include/aqz_gpu.h, without a GPU.
"""
import os
import subprocess

import pytest

from codec_helpers import libzstd, zstd_decode
from test_zstddec_cpu import corpus_records
from zstddec_helpers import MAGIC, OK, inspect, load_golden, write_corpus
from zstdpar_helpers import (assembled_parallel, block_capacity, definers, over_capacity_frame,
                             parallel_scratch_bytes)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "acquire-zarr_amd", "csrc")

pytestmark = pytest.mark.skipif(libzstd() is None, reason="no libzstd")


def parallel_records():
    out = []
    for name, fr, n in assembled_parallel() + [over_capacity_frame()]:
        out.append((f"parallel_{name}", fr, n, OK, zstd_decode(fr, n)))
    return out


def test_new_frames_are_what_they_claim():
    by = {name: (fr, n) for name, fr, n in assembled_parallel()}
    for n in (63, 64, 65, 129):
        assert inspect(by[f"nseq_{n}"][0])["blocks"][0]["nseq"] == n
    assert inspect(by["batch_all_dependent"][0])["blocks"][0]["nseq"] == 81
    assert inspect(by["batch_none_dependent"][0])["blocks"][1]["nseq"] == 64
    for prev in ("compressed", "raw", "rle"):
        kinds = [b["type"] for b in inspect(by[f"rep1_ll0_after_{prev}"][0])["blocks"]]
        assert kinds[-2] == prev and kinds[-1] == "compressed"
    name, fr, n = over_capacity_frame()
    assert len(inspect(fr)["blocks"]) == 3 + block_capacity(n)
    # the chains of the golden frame: treeless blocks whose tree is an earlier block's
    golden, _ = load_golden()
    info = inspect(golden["text_windowed"][0])
    d = definers(info)
    blocks = info["blocks"]
    assert sum(1 for j, use in d.items()
               if blocks[j]["lit_type"] == "treeless" and j - use[0] >= 2) >= 30
    # ... and the built frame: a treeless block and Repeat_Mode tables whose
    # definers lie two blocks back and more, raw blocks between
    info = inspect(by["chain_two_back"][0])
    d = definers(info)
    assert info["blocks"][2]["type"] == info["blocks"][4]["type"] == "raw"
    assert info["blocks"][3]["lit_type"] == "treeless" and d[3] == [0, 1, 1, 1]
    assert info["blocks"][3]["modes"] == ("repeat", "repeat", "repeat")
    assert info["blocks"][5]["modes"] == ("fse", "repeat", "fse") and d[5][2] == 1


def test_parallel_phases_clean_and_equal_to_the_serial_parse(tmp_path):
    exe = str(tmp_path / "zstdpar_sanitize")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++20", *flags, "-I", CSRC,
                        os.path.join(REPO, "tests", "sanitize", "zstdpar_sanitize.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    records = corpus_records() + parallel_records()
    corpus = str(tmp_path / "corpus.bin")
    write_corpus(corpus, records)
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, corpus], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    assert f"clean: {len(records)} records" in r.stdout
    assert "runtime error" not in r.stderr
    got = {}
    for line in r.stdout.splitlines():
        if not line.startswith(("FAIL", "clean")):
            name, st, how = line.rsplit(" ", 2)
            got.setdefault(name, (int(st), how))
    statuses = set()
    for name, fr, _, status, _ in records:
        plain = len(fr) >= 4 and int.from_bytes(fr[:4], "little") == MAGIC
        if status >= 0:
            assert got[name][0] == status, name
            statuses.add(status)
        if not plain:
            continue
        # the fallback: only the frame built to exceed the block table
        if name == "parallel_over_capacity":
            assert got[name] == (OK, "fallback")
        elif status == OK:
            assert got[name] == (OK, "taken"), (name, got[name])
        else:
            assert got[name][1] in ("taken", "fallback"), name
    assert {0, 2, 3, 4} <= statuses
    assert sum(1 for v in got.values() if v[1] == "taken") > 100


def test_scratch_formula_needs_no_gpu():
    import aqz
    Z, P = aqz.DECODE_CODEC_ZSTD, aqz.DECODE_ZSTD_PARALLEL
    assert P == 4
    for n, chunks in ((1, 1), (50, 3), (4095, 2), (4096, 2), (100_003, 7), (600_000, 1),
                      (8 << 20, 64), (0x7fffffef, 2)):
        plain = aqz.decompressor_scratch_bytes(n, chunks, Z)
        pitch = (n + 15) // 16 * 16
        assert plain == chunks * (pitch + min(8, -(-n // 32768)) * min(pitch, 128 * 1024))
        assert aqz.decompressor_scratch_bytes(n, chunks, Z | P) == \
            plain + parallel_scratch_bytes(n, chunks), (n, chunks)
    # the bit alone, and next to the LZ4 family, is refused
    assert aqz.decompressor_scratch_bytes(4096, 2, P) == 0
    assert aqz.decompressor_scratch_bytes(4096, 2, P | aqz.DECODE_CODEC_LZ4) == 0
    assert aqz.decompressor_scratch_bytes(4096, 2, 8 | Z) == 0
    # a reader's estimate follows the decoder's
    from oracle_bindings import SPACE, TIME, U16
    dims = [(TIME, 0, 2, 1), (SPACE, 512, 128, 1), (SPACE, 384, 128, 1)]
    n, bpc = 12, 2 * 128 * 128 * 2
    assert aqz.reader_device_bytes(dims, U16, codecs=Z | P) - \
        aqz.reader_device_bytes(dims, U16, codecs=Z) == parallel_scratch_bytes(bpc, n)
    assert aqz.reader_device_bytes(dims, U16, codecs=P) == 0
