// aqz_lz4dec.hh -- the blosc1 / LZ4 frame parser of the device decoder
// (aqz_decode.hip), compiled for host and device from this one text: the
// header and block-start checks, the stream chain of a block, the LZ4 token
// walk with every bound it enforces, and the byte map of the un-shuffles.
// Only the byte movers differ (the Io argument of lz4_decode): a serial loop
// on the host (tests/sanitize/lz4dec_sanitize.cpp runs this text under a host
// sanitizer), the 64 lanes of a wave on the device.
//
// Format contract: the codec metadata the reference writes into zarr.json
// (array.cpp:340-360: blosc, cname lz4, clevel, shuffle, typesize, blocksize
// 0) promises a blosc1 frame per chunk -- 16-byte header (version,
// versionlz, flags, typesize, nbytes, blocksize, cbytes; flags 0x1 byte
// shuffle, 0x2 memcpyed, 0x4 bit shuffle, 0x10 don't split, bits 5-7 the
// codec), one uint32 start per block, per block one (uint32 csize, bytes)
// record per stream; csize == stream length means stored raw.
#pragma once

#include <cstdint>

#if defined(__HIP__) || defined(__CUDACC__)
#define AQZ_HD __host__ __device__
#else
#define AQZ_HD
#endif

namespace aqz {
namespace dec {

// per-chunk decode status (== AQZ_DECODE_* of aqz_gpu.h)
enum : uint32_t
{
    kOk = 0,
    kSkipped = 1,
    kBadHeader = 2,
    kCorrupt = 3,
    kUnsupported = 4,
    kNotLoaded = 5, // a ranged decode with an empty range: the frame was not looked at
};

constexpr uint32_t kZstdMagic = 0xFD2FB528u;
constexpr uint32_t kSkippableMagic = 0x184D2A50u; // .. 0x184D2A5F
constexpr uint32_t kCodecLz4 = 1; // flags >> 5 (LZ4 and LZ4HC share it)
constexpr uint32_t kCodecZstd = 4;
constexpr uint32_t kMaxSplit = 16; // a block splits into at most 16 streams

AQZ_HD inline uint32_t
rd32(const uint8_t* p)
{
    return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

// Codec families of a decoder (== AQZ_DECODE_CODEC_* of aqz_gpu.h)
constexpr uint32_t kFamilyLz4 = 1, kFamilyZstd = 2;

// Which decoder a frame belongs to, by its first bytes: kFamilyLz4 a blosc1 frame
// of the LZ4 codec, kFamilyZstd a plain zstd (or skippable) frame or a blosc1 frame of the zstd codec,
// 0 anything else.
AQZ_HD inline uint32_t
frame_family(const uint8_t* f, uint64_t frame_bytes)
{
    if (frame_bytes >= 4 && (rd32(f) == kZstdMagic || (rd32(f) & 0xfffffff0u) == kSkippableMagic))
        return kFamilyZstd;
    if (frame_bytes < 16 || f[0] != 2)
        return 0;
    const uint32_t c = uint32_t(f[2]) >> 5;
    return c == kCodecLz4 ? kFamilyLz4 : c == kCodecZstd ? kFamilyZstd : 0u;
}

struct FrameInfo
{
    uint32_t flags, typesize, nbytes, blocksize, cbytes;
    uint32_t nfull, left, nblocks;
    uint32_t memcpyed;
    uint32_t mode; // un-shuffle of a block: 0 none, 1 byte, 2 bit
};

// The 16-byte header of the frame [f, f + frame_bytes) that must decode to
// chunk_bytes.  kOk, or the status the frame gets.  codec: the compressor
// code (flags >> 5) the caller decodes; the zstd decoder (aqz_zstddec.hh)
// passes kCodecZstd for the same container.
AQZ_HD inline uint32_t
parse_header(const uint8_t* f, uint64_t frame_bytes, uint64_t chunk_bytes, FrameInfo& h,
             uint32_t codec = kCodecLz4)
{
    if (frame_bytes >= 4 && rd32(f) == kZstdMagic)
        return kUnsupported; // a plain zstd frame
    if (frame_bytes < 16)
        return kBadHeader;
    if (f[0] != 2)
        return kBadHeader;
    h.flags = f[2];
    h.typesize = f[3];
    h.nbytes = rd32(f + 4);
    h.blocksize = rd32(f + 8);
    h.cbytes = rd32(f + 12);
    if ((h.flags >> 5) != codec)
        return kUnsupported;
    if (h.typesize == 0 || h.nbytes != chunk_bytes || h.cbytes != frame_bytes)
        return kBadHeader;
    h.memcpyed = (h.flags & 0x2u) ? 1u : 0u;
    h.mode = ((h.flags & 0x1u) && h.typesize > 1) ? 1u : (h.flags & 0x4u) ? 2u : 0u;
    h.nfull = h.left = h.nblocks = 0;
    if (h.memcpyed)
        return uint64_t(h.nbytes) + 16 == h.cbytes ? kOk : kBadHeader;
    if (h.blocksize == 0 || h.blocksize % h.typesize != 0)
        return kBadHeader;
    h.nfull = h.nbytes / h.blocksize;
    h.left = h.nbytes % h.blocksize;
    h.nblocks = h.nfull + (h.left ? 1u : 0u);
    if (16 + 4 * uint64_t(h.nblocks) > h.cbytes)
        return kBadHeader;
    return kOk;
}

// Start of block j's records (its bstarts entry); kBadHeader when it leaves
// no room for a record inside the frame.
AQZ_HD inline uint32_t
block_start(const uint8_t* f, const FrameInfo& h, uint32_t j, uint32_t& pos)
{
    pos = rd32(f + 16 + 4 * uint64_t(j));
    if (pos < 16 + 4 * uint64_t(h.nblocks) || uint64_t(pos) + 4 > h.cbytes)
        return kBadHeader;
    return kOk;
}

struct BlockInfo
{
    uint32_t bsize; // bytes of the block
    uint32_t ns;    // streams: typesize (split) or 1
    uint32_t slen;  // bytes of each stream
};

// c-blosc's split rule; the leftover block is never split.
AQZ_HD inline BlockInfo
block_info(const FrameInfo& h, uint32_t j)
{
    BlockInfo b;
    const bool leftover = j >= h.nfull;
    b.bsize = leftover ? h.left : h.blocksize;
    const bool split = !(h.flags & 0x10u) && h.typesize <= kMaxSplit &&
                       h.blocksize / h.typesize >= 128 && !leftover;
    b.ns = split ? h.typesize : 1;
    b.slen = b.bsize / b.ns;
    return b;
}

// A partial decode.  Every block of a blosc1 frame is compressed and shuffled
// on its own, so chunk bytes [lo, hi) need only the blocks that meet them.
struct ByteRange
{
    uint64_t lo, hi; // chunk bytes [lo, hi)
};

// 0: chunk bytes [lo, hi) can be asked of a chunk of chunk_bytes; kNotLoaded:
// the range is empty (nothing is decoded, the frame is not looked at);
// kBadHeader: it is reversed or leaves the chunk.
AQZ_HD inline uint32_t
range_status(ByteRange r, uint64_t chunk_bytes)
{
    if (r.lo > r.hi || r.hi > chunk_bytes)
        return kBadHeader;
    return r.lo == r.hi ? kNotLoaded : kOk;
}

struct BlockRange
{
    uint32_t jlo, jhi; // blocks [jlo, jhi) of the frame
    uint64_t lo, hi;   // the chunk bytes they decode to
};

// The blocks of a parsed (not memcpyed) frame that meet chunk bytes [lo, hi):
// [lo / blocksize, ceil(hi / blocksize)) clipped to nblocks, and the span
// they decode to, [jlo * blocksize, min(jhi * blocksize, nbytes)).  An empty
// or reversed range, and one past the frame's last byte, give no block and an
// empty span.  64-bit arithmetic throughout: blocksize may exceed nbytes, and
// hi + blocksize may exceed 2^32.
AQZ_HD inline BlockRange
blocks_of_range(const FrameInfo& h, uint64_t lo, uint64_t hi)
{
    BlockRange b{ 0, 0, 0, 0 };
    if (lo >= hi || lo >= h.nbytes || h.blocksize == 0 || h.nblocks == 0)
        return b;
    const uint64_t bs = h.blocksize;
    uint64_t jlo = lo / bs;
    uint64_t jhi = hi / bs + (hi % bs ? 1u : 0u);
    if (jhi > h.nblocks)
        jhi = h.nblocks;
    if (jlo >= jhi)
        return b;
    b.jlo = uint32_t(jlo);
    b.jhi = uint32_t(jhi);
    b.lo = jlo * bs;
    b.hi = jhi * bs < h.nbytes ? jhi * bs : uint64_t(h.nbytes);
    return b;
}

// The stream record at pos: its bytes [src, src + csize) inside the frame;
// pos moves to the next record.
AQZ_HD inline uint32_t
next_stream(const uint8_t* f, const FrameInfo& h, uint32_t& pos, uint32_t& src,
            uint32_t& csize)
{
    if (uint64_t(pos) + 4 > h.cbytes)
        return kCorrupt;
    csize = rd32(f + pos);
    if (uint64_t(pos) + 4 + csize > h.cbytes)
        return kCorrupt;
    src = pos + 4;
    pos = src + csize;
    return kOk;
}

// One LZ4 block of n_src bytes that must give exactly n_dst bytes.
//   io.ctl(q)              byte q of the source (q < n_src)
//   io.literals(d, q, n)   out[d .. d+n) = source[q .. q+n)
//   io.match(d, off, n)    out[d + i] = out[d - off + i % off], i < n
// Every call is made with its range already checked: source reads end at
// n_src, output writes at n_dst, and a match never reaches before the
// stream's first byte.
template<typename Io>
AQZ_HD inline uint32_t
lz4_decode(Io& io, uint32_t n_src, uint32_t n_dst)
{
    uint32_t p = 0, d = 0;
    for (;;) {
        if (p >= n_src)
            return kCorrupt;
        const uint32_t token = io.ctl(p++);
        uint32_t ll = token >> 4;
        if (ll == 15) {
            uint32_t b;
            do {
                if (p >= n_src)
                    return kCorrupt;
                b = io.ctl(p++);
                ll += b;
                if (ll > n_dst)
                    return kCorrupt;
            } while (b == 255);
        }
        if (ll > n_src - p || ll > n_dst - d)
            return kCorrupt;
        if (ll)
            io.literals(d, p, ll);
        p += ll;
        d += ll;
        if (p == n_src) // the last sequence has literals only
            return d == n_dst ? kOk : kCorrupt;
        if (n_src - p < 2)
            return kCorrupt;
        const uint32_t off = io.ctl(p) | io.ctl(p + 1) << 8;
        p += 2;
        if (off == 0 || off > d)
            return kCorrupt;
        uint32_t ml = token & 15u;
        if (ml == 15) {
            uint32_t b;
            do {
                if (p >= n_src)
                    return kCorrupt;
                b = io.ctl(p++);
                ml += b;
                if (ml > n_dst)
                    return kCorrupt;
            } while (b == 255);
        }
        ml += 4;
        if (ml > n_dst - d)
            return kCorrupt;
        io.match(d, off, ml);
        d += ml;
    }
}

// Does a block of bsize bytes go through the element-wise un-shuffle?  (A
// bit-shuffled block whose element count is no multiple of 8 was stored as
// it is; the bytes after the last whole element of any block were, as
// c-blosc's shuffles leave them.)
AQZ_HD inline bool
block_is_shuffled(uint32_t bsize, uint32_t ts, uint32_t mode)
{
    const uint32_t ne = bsize / ts;
    if (mode == 1)
        return ne > 0;
    if (mode == 2)
        return ne % 8 == 0 && ne > 0;
    return false;
}

// Byte x of the un-shuffled block from its shuffled bytes s (the inverse of
// c-blosc 1.x's shuffle / bitshuffle of one block).
AQZ_HD inline uint8_t
unshuffled_byte(const uint8_t* s, uint32_t bsize, uint32_t ts, uint32_t mode, uint32_t x)
{
    if (!block_is_shuffled(bsize, ts, mode))
        return s[x];
    const uint32_t ne = bsize / ts;
    if (x >= ne * ts)
        return s[x];
    const uint32_t i = x / ts, jj = x - i * ts;
    if (mode == 1)
        return s[jj * ne + i];
    const uint32_t row = ne / 8;
    uint32_t v = 0;
    for (uint32_t b = 0; b < 8; ++b)
        v |= ((uint32_t(s[(jj * 8 + b) * row + (i >> 3)]) >> (i & 7u)) & 1u) << b;
    return uint8_t(v);
}

} // namespace dec
} // namespace aqz
