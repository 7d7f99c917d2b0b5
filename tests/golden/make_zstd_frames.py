"""Generator of tests/golden/zstd_frames.npz: zstd frames made by libzstd itself
(ZSTD_compress2 with explicit level / windowLog / checksum) and blosc1 frames of
the zstd codec made by c-blosc 1.21, the independent encoders whose output the
device zstd decoder must read.  Run on a CPU host that has both
(codec_helpers.libzstd() and libblosc()); the GPU suite then needs only the
committed file.

    python tests/golden/make_zstd_frames.py

Per case the file holds the frame bytes (frame_<i>), the length it decodes to
and the sha256 of the payload.  The conditions asserted at the end
(zstddec_helpers.conditions: every literals kind, weight coding, table mode and
frame-header shape the decoder must accept) are re-asserted on the committed
file by tests/test_zstddec_cpu.py.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from codec_helpers import camera_like, libblosc, libblosc_decode, libzstd  # noqa: E402
from zstddec_helpers import (GOLDEN, conditions, inspect, reference_decode, sha256,  # noqa: E402
                             zstd_compress2)

DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
MAX_FILE = 256 * 1024
WORDS = (b"chunk", b"shard", b"zarr", b"pixel", b"frame", b"the", b"of", b"and", b"stream",
         b"layer", b"level", b"codec", b"camera", b"to", b"a", b"in")


def text(rng, n):
    out = b""
    while len(out) < n:
        out += WORDS[int(rng.integers(len(WORDS)))] + b" "
    return out[:n]


def records(rng, n, n_random, fixed: bytes):
    return b"".join(rng.integers(0, 256, n_random, dtype=np.uint8).tobytes() + fixed
                    for _ in range(n))


def sparse(rng, n, hits):
    a = np.zeros(n, np.uint8)
    a[rng.integers(0, n, hits)] = 7
    return a.tobytes()


def blosc(data: bytes, ts: int, shuffle: int, blocksize: int = 0, clevel: int = 5) -> bytes:
    L = libblosc()
    out = C.create_string_buffer(len(data) + 16)
    n = L.blosc_compress_ctx(clevel, shuffle, ts, len(data), data, out, len(data) + 16, b"zstd",
                             blocksize, 1)
    assert n > 0
    return out.raw[:n]


def payload(rng, kind: str, ts: int, n_px: int) -> bytes:
    dt = DT[ts]
    if kind == "camera":
        a = camera_like(rng, n_px, dt, level=1000.0, noise=30.0, amp=200.0)
    elif kind == "sparse":
        a = np.zeros(n_px, dt)
        a[rng.integers(0, n_px, max(1, n_px // 50))] = 7
    else:
        a = (np.arange(n_px) % 251).astype(dt)
    return a.tobytes()


def main():
    assert libzstd() is not None and libblosc() is not None, "libzstd and c-blosc are needed"
    rng = np.random.default_rng(20261020)
    cases = []  # (name, payload, frame)

    def plain(name, data, level, window_log=0, checksum=False):
        cases.append((name, data, zstd_compress2(data, level, window_log, checksum)))

    plain("text_1stream", text(rng, 200), 3)
    plain("sparse_direct_treeless", sparse(rng, 200000, 4000), 3)
    plain("text_windowed", text(rng, 40000), 3, window_log=10, checksum=True)
    plain("zeros_rle_block", bytes(200000), 3)
    plain("random_raw_block", rng.integers(0, 256, 300, dtype=np.uint8).tobytes(), 3)
    plain("five_bytes", b"hello", 3)
    plain("empty", b"", 3)
    plain("records_rle_tables", records(rng, 9000, 2, b"0123456789abcdefghijklmnopqrst"), 19)
    # quiet camera frames at level 19: FSE-compressed weights, > 32512 sequences
    # in one block (the 3-byte count)
    plain("camera_fse_weights", camera_like(rng, 65536, np.uint16, noise=3.0).tobytes(), 19)
    for ts in (1, 2, 4, 8):
        for sh in (0, 1, 2):
            kind = "camera" if (ts, sh) in ((2, 1), (4, 2)) else "ramp" if sh == 0 else "sparse"
            data = payload(rng, kind, ts, 3000 // ts)
            cases.append((f"blosc_ts{ts}_sh{sh}", data, blosc(data, ts, sh)))
    data = payload(rng, "camera", 2, 50)
    cases.append(("blosc_tiny_memcpyed", data, blosc(data, 2, 1)))
    # a forced block size b becomes b for zstd: full blocks and a leftover
    data = payload(rng, "sparse", 2, (16384 * 3 + 5000) // 2)
    cases.append(("blosc_ts2_sh1_blocks", data, blosc(data, 2, 1, 16384)))
    data = payload(rng, "ramp", 4, (16384 * 2 + 1236) // 4)
    cases.append(("blosc_ts4_sh2_blocks", data, blosc(data, 4, 2, 16384)))
    data = payload(rng, "ramp", 1, 16384 * 2 + 777)
    cases.append(("blosc_ts1_sh0_blocks", data, blosc(data, 1, 0, 16384)))
    # the default block size: one block above 32 KiB (the scratch path)
    data = payload(rng, "sparse", 2, 60000)
    cases.append(("blosc_ts2_sh1_one_block", data, blosc(data, 2, 1)))
    data = payload(rng, "sparse", 4, 25000)
    cases.append(("blosc_ts4_sh2_one_block", data, blosc(data, 4, 2)))

    out, names, nbytes, shas = {}, [], [], []
    for i, (name, data, fr) in enumerate(cases):
        assert reference_decode(fr, len(data)) == data, name
        if name.startswith("blosc_"):
            assert libblosc_decode(fr) == data, name
            what = "flags %#04x blocksize %d" % (fr[2], int.from_bytes(fr[8:12], "little"))
        else:
            info = inspect(fr)
            what = "%d blocks" % len(info["blocks"])
        out[f"frame_{i}"] = np.frombuffer(fr, dtype=np.uint8)
        names.append(name)
        nbytes.append(len(data))
        shas.append(sha256(data))
        print(f"{name:28s} {len(data):7d} -> {len(fr):7d}  {what}")
    conditions({n: (bytes(out[f"frame_{i}"]), nbytes[i]) for i, n in enumerate(names)})
    out["names"] = np.array(names)
    out["nbytes"] = np.array(nbytes, dtype=np.uint64)
    out["sha256"] = np.array(shas)
    np.savez(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print(f"{GOLDEN}: {size} bytes")
    assert size <= MAX_FILE, size


if __name__ == "__main__":
    main()
