"""Payloads that put the device zstd / LZ4 encoders on their edges
(test_encoder_payloads_cpu.py, test_gpu_zstd_paths.py): each generator is
kind(rng, nbytes) -> uint8[nbytes], deterministic in the rng's seed and exact
in length for any nbytes >= 1 (a pattern longer than nbytes is truncated, a
shorter one is laid again with fresh random bytes).  Pure numpy.

What each kind is for:
  zeros const random camera dim ramp251   the baseline of the other suites
  two_values_50 / _01   two byte values, p = 0.5 and 0.01: 1-bit Huffman codes
  nibble_uniform        the 16 byte values 0..15, equiprobable: 15 equal
                        weights, a direct tree description
  skewed_deep           256 symbols, counts falling like Fibonacci numbers over
                        a floor: an unlimited Huffman code is deeper than 11
                        bits (the depth limiter runs), symbols above 128 (the
                        weights are FSE-compressed)
  text                  bytes 32..126, words of a small list
  period_P              P random bytes repeated: matches that end at and cross
                        the 4 KiB parse units and 8 KiB blocks, distances
                        beyond a unit
  short_and_long        4-byte dictionary words + 1 fresh byte, then a 4 KiB
                        block repeated: match-length codes in two regions more
                        than 24 codes apart
  run_ladder            runs of one value closed by a fresh byte, lengths on
                        the ML / LL code-table steps and LZ4's 15 / 15 + 255
  literal_ladder        an 8-byte copy of earlier bytes after k fresh bytes, k
                        on the LL code-table steps and across a parse unit
  raw_head raw_middle   24 KiB of random bytes first / in the middle, dim
                        camera data elsewhere: raw blocks before and between
                        the blocks with sequences
  tail_copy_K           random bytes whose last K repeat earlier ones: a match
                        that ends at the last byte

TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import zlib

import numpy as np

PERIODS = (1, 3, 4, 5, 251, 4095, 4096, 4099, 8192 + 17)
TAILS = (7, 5, 4, 3)
RUN_LENGTHS = (list(range(1, 41)) + list(range(63, 67)) + list(range(127, 132)) +
               list(range(255, 260)) + list(range(270, 276)) + list(range(511, 517)) +
               list(range(1023, 1027)) + list(range(4090, 4101)))
LITERAL_GAPS = (list(range(0, 71)) + list(range(127, 131)) + [4000] +
                list(range(4095, 4098)) + [8000])
WORDS = ("chunk", "frame", "zarr", "the", "of", "a", "stream", "shard", "level", "pixel", "and",
         "camera", "is", "to", "in", "array", "index", "write", "dimension", "it")
RAW_SPAN = 3 * 8192


def _random(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def _camera(rng, n, **kw):
    level, noise, amp = kw.get("level", 1000.0), kw.get("noise", 30.0), kw.get("amp", 200.0)
    n_px = (n + 1) // 2
    x = np.arange(n_px, dtype=np.float64)
    v = level + amp * np.sin(x / 977.0) + rng.normal(0.0, noise, n_px)
    return np.clip(v, 0, 65535).astype(np.uint16).view(np.uint8)[:n].copy()


def _cycled(rng, n, lap):
    """lap(rng) -> uint8 pattern, laid again until n bytes are there."""
    parts, have = [], 0
    while have < n:
        a = lap(rng)
        parts.append(a)
        have += a.size
    return np.concatenate(parts)[:n]


def zeros(rng, n):
    return np.zeros(n, np.uint8)


def const(rng, n):
    return np.full(n, 0xA5, np.uint8)


def random(rng, n):
    return _random(rng, n)


def camera(rng, n):
    return _camera(rng, n)


def dim(rng, n):
    return _camera(rng, n, level=100.0, noise=3.0, amp=0.0)


def ramp251(rng, n):
    return (np.arange(n) % 251).astype(np.uint8)


def _two_values(p):
    def kind(rng, n):
        return np.where(rng.random(n) < p, np.uint8(0xEE), np.uint8(0x11))
    return kind


def nibble_uniform(rng, n):
    # every 16 bytes a permutation of the 16 symbols: equal counts exactly
    groups = (n + 15) // 16
    perm = np.argsort(rng.random((groups, 16)), axis=1).astype(np.uint8)
    return perm.reshape(-1)[:n].copy()      # values 0..15: 15 weights, all equal


def skewed_deep(rng, n):
    phi = (1 + 5 ** 0.5) / 2
    p = phi ** -np.arange(256, dtype=np.float64)
    p = p / p.sum() * (1 - 1 / 16) + 1 / 16 / 256   # the floor: every symbol appears
    value = rng.permutation(256).astype(np.uint8)   # rank -> byte value
    return value[rng.choice(256, size=n, p=p / p.sum())]


def text(rng, n):
    idx = rng.integers(0, len(WORDS), n // 2 + 1)
    s = " ".join(WORDS[i] for i in idx).encode()
    assert len(s) >= n
    return np.frombuffer(s[:n], np.uint8).copy()


def _period(p):
    def kind(rng, n):
        return np.resize(_random(rng, p), n)
    return kind


def short_and_long(rng, n):
    half = n // 2
    words = _random(rng, 64 * 4).reshape(64, 4)
    rec = (half + 4) // 5
    a = np.empty((rec, 5), np.uint8)
    a[:, :4] = words[rng.integers(0, 64, rec)]
    a[:, 4] = _random(rng, rec)
    return np.concatenate([a.reshape(-1)[:half], np.resize(_random(rng, 4096), n - half)])


def run_ladder(rng, n):
    def lap(rng):
        total = sum(RUN_LENGTHS) + len(RUN_LENGTHS)
        a = np.full(total, 0x5A, np.uint8)
        ends = np.cumsum(np.asarray(RUN_LENGTHS) + 1) - 1
        a[ends] = _random(rng, len(ends))
        return a
    return _cycled(rng, n, lap)


def literal_ladder(rng, n):
    def lap(rng):
        parts = [_random(rng, 16)]
        last8 = parts[0][-8:]
        for k in LITERAL_GAPS:
            parts += [_random(rng, k), last8]   # the 8 bytes before the fresh ones, again
        return np.concatenate(parts)
    return _cycled(rng, n, lap)


def raw_head(rng, n):
    a = dim(rng, n)
    k = min(n, RAW_SPAN)
    a[:k] = _random(rng, k)
    return a


def raw_middle(rng, n):
    a = dim(rng, n)
    s = n // 2 // 8192 * 8192
    k = min(n - s, RAW_SPAN)
    a[s:s + k] = _random(rng, k)
    return a


def _tail_copy(k):
    def kind(rng, n):
        a = _random(rng, n)
        if n >= 2 * k:
            s = max(0, n - k - 64)
            a[n - k:] = a[s:s + k]
        return a
    return kind


KINDS = dict(zeros=zeros, const=const, random=random, camera=camera, dim=dim, ramp251=ramp251,
             two_values_50=_two_values(0.5), two_values_01=_two_values(0.01),
             nibble_uniform=nibble_uniform, skewed_deep=skewed_deep, text=text)
KINDS.update({f"period_{p}": _period(p) for p in PERIODS})
KINDS.update(short_and_long=short_and_long, run_ladder=run_ladder, literal_ladder=literal_ladder,
             raw_head=raw_head, raw_middle=raw_middle)
KINDS.update({f"tail_copy_{k}": _tail_copy(k) for k in TAILS})
NAMES = tuple(KINDS)
LZ4_NAMES = ("run_ladder", "literal_ladder", "two_values_50", "two_values_01") + \
    tuple(f"period_{p}" for p in PERIODS) + tuple(f"tail_copy_{k}" for k in TAILS)


def make(name: str, nbytes: int, seed: int = 0) -> np.ndarray:
    """The payload of a kind: the rng is seeded by (seed, kind), so a kind's
    bytes do not depend on which other kinds are made."""
    rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
    a = KINDS[name](rng, nbytes)
    assert a.dtype == np.uint8 and a.shape == (nbytes,), (name, a.dtype, a.shape)
    return a


def stack(nbytes: int, seed: int = 0, names=NAMES) -> np.ndarray:
    """(len(names), nbytes): every kind as one chunk of a run."""
    return np.stack([make(k, nbytes, seed) for k in names])
