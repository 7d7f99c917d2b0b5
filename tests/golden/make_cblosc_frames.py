"""Generator of tests/golden/cblosc_lz4_frames.npz: blosc1 frames made by c-blosc
1.21 itself (codec lz4, clevel 5), the independent encoder whose output the device
decoder must read.  Run on a CPU host that has c-blosc (codec_helpers.libblosc());
the GPU suite then needs only the committed file.

    python tests/golden/make_cblosc_frames.py

Per case the file holds the frame bytes (frame_<i>), the typesize, the shuffle
mode and the sha256 of the original payload.  Payloads are compressible
(camera-like, sparse, ramp) so the file stays at or below 256 KiB.  The
conditions asserted at the end are re-asserted on the committed file by
tests/test_decoder_cpu.py.
"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from codec_helpers import camera_like, libblosc, libblosc_decode, oracle_decode  # noqa: E402
from decoder_helpers import GOLDEN, props, sha256  # noqa: E402

DT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
MAX_FILE = 256 * 1024


def compress(data: bytes, ts: int, shuffle: int, blocksize: int = 0, clevel: int = 5) -> bytes:
    L = libblosc()
    out = C.create_string_buffer(len(data) + 16)
    n = L.blosc_compress_ctx(clevel, shuffle, ts, len(data), data, out, len(data) + 16, b"lz4",
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


# (name, kind, typesize, shuffle, pixels, forced blocksize)
CASES = [(f"camera_ts{ts}_sh{sh}", "camera", ts, sh, 3000 // ts, 0)
         for ts in (1, 2, 4, 8) for sh in (0, 1, 2)]
CASES += [
    ("tiny_memcpyed", "camera", 2, 1, 50, 0),            # below c-blosc's 128-byte floor
    ("few_elements_dont_split", "ramp", 4, 1, 100, 0),   # < 128 elements: one stream
    ("camera_raw_stream", "camera", 2, 1, 20000, 0),     # the noisy low byte is stored raw
    # c-blosc turns a forced block size b into max(b * typesize, 64 KiB)
    ("split_two_full_and_leftover", "sparse", 2, 1, 75000, 32768),
    ("split_bitshuffle_leftover", "ramp", 4, 2, 40000, 16384),
    ("odd_leftover_no_shuffle", "ramp", 1, 0, 70001, 16384),
    ("long_streams", "ramp", 2, 1, 300000, 262144),      # 128 KiB streams: not in LDS
    ("long_streams_bitshuffle", "sparse", 2, 2, 200000, 0),
    ("long_block_one_stream", "sparse", 1, 0, 150000, 0),
]


def main():
    assert libblosc() is not None, "c-blosc is needed to make this fixture"
    rng = np.random.default_rng(20261020)
    out = {}
    names, tss, shs, shas, all_props = [], [], [], [], []
    for i, (name, kind, ts, sh, n_px, bs) in enumerate(CASES):
        data = payload(rng, kind, ts, n_px)
        fr = compress(data, ts, sh, bs)
        assert oracle_decode(fr) == data and libblosc_decode(fr) == data, name
        out[f"frame_{i}"] = np.frombuffer(fr, dtype=np.uint8)
        names.append(name)
        tss.append(ts)
        shs.append(sh)
        shas.append(sha256(data))
        p = props(fr)
        all_props.append(p)
        print(f"{name:32s} {len(data):7d} -> {len(fr):7d}  flags {p['flags']:#04x} "
              f"full/split {p['split_full_blocks']} leftover {p['leftover']} "
              f"raw {p['raw_stream']} max stream {p['max_stream']}")
    check(tss, shs, all_props)
    out["names"] = np.array(names)
    out["typesize"] = np.array(tss, dtype=np.uint32)
    out["shuffle"] = np.array(shs, dtype=np.uint32)
    out["sha256"] = np.array(shas)
    np.savez(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print(f"{GOLDEN}: {size} bytes")
    assert size <= MAX_FILE, size


def check(tss, shs, all_props):
    """The fixture's stated conditions."""
    assert set(tss) >= {1, 2, 4, 8}
    assert set(shs) >= {0, 1, 2}
    assert any(p["memcpyed"] for p in all_props)
    assert any(p["dont_split"] for p in all_props)
    assert any(p["split_full_blocks"] >= 2 and p["leftover"] for p in all_props)
    assert any(p["raw_stream"] and not p["memcpyed"] for p in all_props)
    assert any(p["max_stream"] > 65536 for p in all_props)


if __name__ == "__main__":
    main()
