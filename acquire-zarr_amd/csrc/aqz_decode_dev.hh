// aqz_decode_dev.hh -- device helpers the decoder kernels share
// (aqz_decode.hip, aqz_zstddec.hip): the frame reference of a run, the
// store-or-compare byte emitters and the un-shuffle of one decoded block.
#pragma once

#include "aqz_decode.hh"

namespace aqz {
namespace {

__device__ __forceinline__ uint32_t
uni(uint32_t v)
{
    return uint32_t(__builtin_amdgcn_readfirstlane(int(v)));
}

__device__ __forceinline__ uint64_t
load8(const uint8_t* s)
{
    if ((reinterpret_cast<uintptr_t>(s) & 7u) == 0)
        return *reinterpret_cast<const uint64_t*>(s);
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        v |= uint64_t(s[k]) << (8 * k);
    return v;
}

// 8 decoded bytes for o: stored, or (kCompare) compared with what is there
template<bool kCompare>
__device__ __forceinline__ void
emit8(uint8_t* o, uint64_t v, bool& diff)
{
    if (kCompare) {
        diff |= load8(o) != v;
    } else if ((reinterpret_cast<uintptr_t>(o) & 7u) == 0) {
        *reinterpret_cast<uint64_t*>(o) = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
            o[k] = uint8_t(v >> (8 * k));
    }
}

template<bool kCompare>
__device__ __forceinline__ void
emit1(uint8_t* o, uint8_t v, bool& diff)
{
    if (kCompare)
        diff |= *o != v;
    else
        *o = v;
}

// o[0, n) = s[0, n) (s == nullptr: zeros), by all `nt` threads
template<bool kCompare>
__device__ __forceinline__ void
copy_bytes(uint8_t* o, const uint8_t* s, uint32_t n, uint32_t tid, uint32_t nt, bool& diff)
{
    const uint32_t n8 = n / 8;
    for (uint32_t u = tid; u < n8; u += nt)
        emit8<kCompare>(o + 8 * u, s ? load8(s + 8 * u) : 0ull, diff);
    for (uint32_t x = n8 * 8 + tid; x < n; x += nt)
        emit1<kCompare>(o + x, s ? s[x] : uint8_t(0), diff);
}

// 8x8 bit transpose: byte k of the result holds bit k of every input byte
// (input byte b -> result bit b).
__device__ __forceinline__ uint64_t
transpose8(uint64_t x)
{
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;
    x = x ^ t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull;
    x = x ^ t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull;
    x = x ^ t ^ (t << 28);
    return x;
}

// The element-wise un-shuffle of groups of 8 elements of TS bytes: thread
// -> group g, 8 * TS contiguous output bytes.  Returns the bytes covered.
template<uint32_t TS, bool kCompare>
__device__ __forceinline__ uint32_t
unshuffle_units(const uint8_t* s, uint8_t* o, uint32_t ne, bool bit, uint32_t tid,
                uint32_t nt, bool& diff)
{
    const uint32_t ng = ne / 8;
    for (uint32_t g = tid; g < ng; g += nt) {
        // output byte k * TS + jj = byte jj of element 8g + k.  The jj loop
        // stays rolled (one plane set in registers at a time); the word of
        // w a byte lands in depends on k alone, so w stays in registers.
        uint64_t w[TS] = {};
#pragma unroll 1
        for (uint32_t jj = 0; jj < TS; ++jj) {
            uint64_t t; // byte k of t = byte jj of element 8g + k
            if (bit) {
                uint64_t x = 0;
#pragma unroll
                for (uint32_t b = 0; b < 8; ++b)
                    x |= uint64_t(s[(jj * 8 + b) * ng + g]) << (8 * b);
                t = transpose8(x);
            } else {
                t = load8(s + jj * ne + 8 * g);
            }
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k)
                w[(k * TS) >> 3] |= ((t >> (8 * k)) & 0xffull) << (8 * (((k * TS) & 7u) + jj));
        }
#pragma unroll
        for (uint32_t i = 0; i < TS; ++i)
            emit8<kCompare>(o + (g * TS + i) * 8, w[i], diff);
    }
    return ng * 8 * TS;
}

// One decoded block s (shuffled as the frame says) -> its chunk bytes at o.
template<bool kCompare>
__device__ __forceinline__ void
unshuffle_block(const uint8_t* s, uint8_t* o, uint32_t bsize, uint32_t ts, uint32_t mode,
                uint32_t tid, uint32_t nt, bool& diff)
{
    if (!dec::block_is_shuffled(bsize, ts, mode)) {
        copy_bytes<kCompare>(o, s, bsize, tid, nt, diff);
        return;
    }
    const uint32_t ne = bsize / ts;
    const bool bit = mode == 2;
    uint32_t done = 0;
    switch (ts) {
        case 1:
            done = unshuffle_units<1, kCompare>(s, o, ne, bit, tid, nt, diff);
            break;
        case 2:
            done = unshuffle_units<2, kCompare>(s, o, ne, bit, tid, nt, diff);
            break;
        case 4:
            done = unshuffle_units<4, kCompare>(s, o, ne, bit, tid, nt, diff);
            break;
        case 8:
            done = unshuffle_units<8, kCompare>(s, o, ne, bit, tid, nt, diff);
            break;
        default:
            break;
    }
    // other type sizes, the elements after the last group of 8 and the
    // bytes after the last element
    for (uint32_t x = done + tid; x < bsize; x += nt)
        emit1<kCompare>(o + x, dec::unshuffled_byte(s, bsize, ts, mode, x), diff);
}

// Frame q of the run: its bytes and the chunk it decodes to.  False (with
// the frame's status in st) when the offsets do not describe a frame.
struct FrameRef
{
    const uint8_t* f;
    uint64_t len;
    uint8_t* out;
};

__device__ __forceinline__ bool
frame_ref(const DecodeParams& p, uint32_t q, FrameRef& r)
{
    const uint64_t o0 = p.offsets[q], o1 = p.offsets[q + 1];
    const uint32_t slot = p.order ? p.order[q] : q;
    if (o1 < o0 || o1 > p.frames_bytes || o1 - o0 > 0xffffffffull || slot >= p.n_chunks)
        return false;
    r.f = p.frames + o0;
    r.len = o1 - o0;
    r.out = p.dst + uint64_t(slot) * p.pitch;
    return true;
}

// the span frame q of a ranged run was decoded over (written by one thread)
__device__ __forceinline__ void
put_span(const RangedParams& rp, uint32_t q, uint64_t lo, uint64_t hi)
{
    if (rp.spans) {
        rp.spans[q].lo = lo;
        rp.spans[q].hi = hi;
    }
}

// Workgroups per chunk of a ranged run: one per kDecodeLdsBytes of the longest
// range and one more for a range that straddles a group edge, `cap` at most.
inline uint32_t
ranged_passes(uint64_t chunk_bytes, uint64_t max_range_bytes, uint32_t cap)
{
    const uint64_t bytes =
      max_range_bytes && max_range_bytes < chunk_bytes ? max_range_bytes : chunk_bytes;
    const uint64_t passes = (bytes + kDecodeLdsBytes - 1) / kDecodeLdsBytes + 1;
    return passes > cap ? cap : uint32_t(passes);
}

} // namespace
} // namespace aqz
