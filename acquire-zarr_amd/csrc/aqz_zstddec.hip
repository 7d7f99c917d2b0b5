// aqz_zstddec.hip -- zstd decoding (RFC 8878) of frames resident in HBM on
// gfx950: plain zstd frames and blosc1 frames whose streams are zstd frames.
// The parse and every bound: aqz_zstddec.hh (shared with the host); the
// blosc1 container: aqz_lz4dec.hh.
//
//   zstd_decode   grid (frame, pass), one wave per workgroup.  A plain zstd
//                 frame is decoded by pass 0; the blocks of a blosc1 frame
//                 are dealt round-robin to the passes (they are independent
//                 zstd frames).  The wave walks its zstd frame serially: the
//                 Huffman / FSE tables live in LDS, the four Huffman streams
//                 of a literals section decode on four lanes into the
//                 (chunk, pass) literal slot in global memory, the sequence
//                 decode is wave-uniform, and the 64 lanes move literal and
//                 match bytes.
//                 Matches read back what earlier sequences stored to global
//                 memory (any distance, across blocks): a workgroup-scope
//                 fence separates those stores from the dependent loads, as
//                 on the LZ4 scratch path, issued only when a match's source
//                 reaches into bytes stored since the last fence.
//                 Output: straight into the destination chunk for plain
//                 frames and unshuffled blosc frames; shuffled blosc blocks,
//                 and everything in compare mode, go to the chunk's scratch
//                 slot.
//   zstd_finish   un-shuffles (or compares) what zstd_decode left in the
//                 scratch slots.
#include "aqz_decode.hh"
#include "aqz_decode_dev.hh"
#include "aqz_zstddec.hh"

namespace aqz {
namespace {

constexpr uint32_t kFinishThreads = 256;
constexpr uint32_t kFinishPiece = 64 * 1024; // bytes of a plain frame per workgroup step

__device__ __forceinline__ uint32_t
pick4(const uint32_t (&a)[4], uint32_t k)
{
    return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3];
}

// The byte movers of one wave for zdec::zstd_decode_frame.  out and lit are
// global memory; a lane re-reads bytes other lanes have stored, so a
// workgroup-scope fence separates stores from dependent loads: after the
// Huffman literals are written, and before a match whose source reaches into
// bytes stored since the last fence (out[clean ..)).
struct WaveZIo
{
    const uint8_t* src;
    uint8_t* out;
    uint8_t* lit;
    uint32_t lane;
    uint32_t clean = 0;

    __device__ __forceinline__ void sync()
    {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    }

    __device__ __forceinline__ void copy(uint8_t* o, const uint8_t* s, uint32_t n)
    {
        // four independent loads in flight per lane
        for (uint32_t i = lane; i < n; i += 256) {
            const bool b1 = i + 64 < n, b2 = i + 128 < n, b3 = i + 192 < n;
            const uint8_t v0 = s[i];
            const uint8_t v1 = b1 ? s[i + 64] : uint8_t(0);
            const uint8_t v2 = b2 ? s[i + 128] : uint8_t(0);
            const uint8_t v3 = b3 ? s[i + 192] : uint8_t(0);
            o[i] = v0;
            if (b1)
                o[i + 64] = v1;
            if (b2)
                o[i + 128] = v2;
            if (b3)
                o[i + 192] = v3;
        }
    }

    __device__ __forceinline__ uint32_t huf(const uint8_t* f, const zdec::HufJob& j,
                                            const uint16_t* tab, uint32_t log)
    {
        uint32_t e = dec::kOk;
        if (lane < j.ns)
            e = zdec::huf_decode_stream(f + pick4(j.src, lane), pick4(j.len, lane), tab, log,
                                        lit + pick4(j.dst, lane), pick4(j.cnt, lane));
        uint32_t worst = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ek = uint32_t(__builtin_amdgcn_readlane(int(e), k));
            worst = ek > worst ? ek : worst;
        }
        sync();
        return worst;
    }

    __device__ __forceinline__ void copy_src(uint32_t d, uint32_t q, uint32_t n)
    {
        copy(out + uni(d), src + uni(q), uni(n));
    }

    __device__ __forceinline__ void copy_lit(uint32_t d, uint32_t i, uint32_t n)
    {
        copy(out + uni(d), lit + uni(i), uni(n));
    }

    __device__ __forceinline__ void fill(uint32_t d, uint32_t v, uint32_t n)
    {
        uint8_t* o = out + uni(d);
        const uint8_t b = uint8_t(uni(v));
        n = uni(n);
        for (uint32_t i = lane; i < n; i += 64)
            o[i] = b;
    }

    // every byte read lies before out + d: written by an earlier call
    __device__ __forceinline__ void match(uint32_t d, uint32_t off, uint32_t n)
    {
        off = uni(off);
        n = uni(n);
        d = uni(d);
        // the bytes read: out[d - off, d - off + min(n, off))
        if (d - off + (n < off ? n : off) > clean) {
            sync();
            clean = d;
        }
        uint8_t* o = out + d;
        const uint8_t* m = o - off;
        if (off >= n) {
            for (uint32_t i = lane; i < n; i += 64)
                o[i] = m[i];
        } else {
            // overlapping: out[d + i] = out[d - off + i % off]
            uint32_t r = lane % off;
            const uint32_t step = 64u % off;
            for (uint32_t i = lane; i < n; i += 64) {
                o[i] = m[r];
                r += step;
                if (r >= off)
                    r -= off;
            }
        }
    }
};

// Is frame q staged in its scratch slot (and finished by zstd_finish)?
template<bool kCompare>
__device__ __forceinline__ bool
staged(bool plain, uint32_t mode)
{
    return kCompare || (!plain && mode != 0);
}

template<bool kCompare>
__global__ void __launch_bounds__(64)
zstd_decode(DecodeParams p)
{
    __shared__ zdec::Tables s_t;
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    // frames that do not exist, zero-length frames and frames of other
    // codecs are blosc_decode's
    if (!frame_ref(p, q, r) || r.len == 0 || dec::frame_family(r.f, r.len) != dec::kFamilyZstd)
        return;
    if (p.zfr && p.zfr[2 * q] != 0) // decoded (or refused) by the parallel path
        return;
    const uint32_t len = uint32_t(r.len);
    uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    uint8_t* lit = p.zlit + (uint64_t(q) * p.zpasses + blockIdx.y) * p.zlit_pitch;
    const uint32_t magic = dec::rd32(r.f);
    if (magic == dec::kZstdMagic || (magic & 0xfffffff0u) == dec::kSkippableMagic) {
        if (blockIdx.y != 0)
            return;
        WaveZIo io{ r.f, staged<kCompare>(true, 0) ? scr : r.out, lit, lane };
        const uint32_t e = zdec::zstd_decode_frame(io, r.f, len, uint32_t(p.chunk_bytes), s_t);
        if (e != dec::kOk && lane == 0)
            atomicMax(&p.status[q], e);
        return;
    }
    dec::FrameInfo h;
    const uint32_t st = dec::parse_header(r.f, r.len, p.chunk_bytes, h, dec::kCodecZstd);
    if (st != dec::kOk) {
        if (blockIdx.y == 0 && lane == 0)
            atomicMax(&p.status[q], st);
        return;
    }
    if (h.memcpyed) {
        bool diff = false;
        const uint64_t span = uint64_t(gridDim.y) * kDecodeLdsBytes;
        for (uint64_t b = uint64_t(blockIdx.y) * kDecodeLdsBytes; b < h.nbytes; b += span) {
            const uint64_t left = h.nbytes - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<kCompare>(r.out + b, r.f + 16 + b, n, lane, 64, diff);
        }
        if (kCompare && diff)
            p.bad[q] = 1;
        return;
    }
    uint8_t* base = staged<kCompare>(false, h.mode) ? scr : r.out;
    uint32_t err = dec::kOk;
    for (uint32_t j = blockIdx.y; j < h.nblocks && err == dec::kOk; j += gridDim.y) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        uint32_t pos = 0;
        err = dec::block_start(r.f, h, j, pos);
        for (uint32_t s = 0; s < bi.ns && err == dec::kOk; ++s) {
            uint32_t src = 0, csz = 0;
            err = dec::next_stream(r.f, h, pos, src, csz);
            if (err != dec::kOk)
                break;
            src = uni(src);
            csz = uni(csz);
            WaveZIo io{ r.f + src, base + uint64_t(j) * h.blocksize + uint64_t(s) * bi.slen, lit,
                        lane };
            if (csz == bi.slen) { // stored raw
                if (bi.slen)
                    io.copy_src(0, 0, bi.slen);
            } else {
                err = zdec::zstd_decode_frame(io, r.f + src, csz, bi.slen, s_t);
            }
        }
    }
    if (err != dec::kOk && lane == 0)
        atomicMax(&p.status[q], err);
}

template<bool kCompare>
__global__ void __launch_bounds__(kFinishThreads)
zstd_finish(DecodeParams p)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0 || dec::frame_family(r.f, r.len) != dec::kFamilyZstd)
        return;
    if (p.status[q] != dec::kOk) // written by zstd_decode, complete before this kernel
        return;
    const uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    bool diff = false;
    if (dec::rd32(r.f) == dec::kZstdMagic) {
        if (!staged<kCompare>(true, 0))
            return;
        const uint64_t span = uint64_t(gridDim.y) * kFinishPiece;
        for (uint64_t b = uint64_t(blockIdx.y) * kFinishPiece; b < p.chunk_bytes; b += span) {
            const uint64_t left = p.chunk_bytes - b;
            const uint32_t n = left < kFinishPiece ? uint32_t(left) : kFinishPiece;
            copy_bytes<kCompare>(r.out + b, scr + b, n, tid, kFinishThreads, diff);
        }
    } else {
        dec::FrameInfo h;
        if (dec::parse_header(r.f, r.len, p.chunk_bytes, h, dec::kCodecZstd) != dec::kOk ||
            h.memcpyed || !staged<kCompare>(false, h.mode))
            return;
        for (uint32_t j = blockIdx.y; j < h.nblocks; j += gridDim.y) {
            const dec::BlockInfo bi = dec::block_info(h, j);
            unshuffle_block<kCompare>(scr + uint64_t(j) * h.blocksize,
                                      r.out + uint64_t(j) * h.blocksize, bi.bsize, h.typesize,
                                      h.mode, tid, kFinishThreads, diff);
        }
    }
    if (kCompare && diff)
        p.bad[q] = 1;
}

// ---- ranged decode ----------------------------------------------------------
// zstd_decode and zstd_finish over the blocks of a blosc1-zstd frame that meet
// a byte range (aqz_decode.hh, RangedParams; no compare mode).  Kernels of
// their own, so that the code of a full run is what it was.  The blocks of a
// frame are independent zstd frames: blocks [jlo, jhi) are dealt to the
// passes from jlo on.  A plain zstd frame is decoded whole, as in a full run
// (its matches reach across blocks), and reports the whole chunk.  Empty and
// bad ranges got their status from blosc_decode_ranged and are left alone.
__global__ void __launch_bounds__(64)
zstd_decode_ranged(RangedParams rp)
{
    __shared__ zdec::Tables s_t;
    const DecodeParams& p = rp.p;
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const bool lead = blockIdx.y == 0 && lane == 0;
    const dec::ByteRange want = rp.ranges[q];
    if (dec::range_status(want, p.chunk_bytes) != dec::kOk)
        return;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0 || dec::frame_family(r.f, r.len) != dec::kFamilyZstd)
        return;
    const uint32_t len = uint32_t(r.len);
    uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    uint8_t* lit = p.zlit + (uint64_t(q) * p.zpasses + blockIdx.y) * p.zlit_pitch;
    const uint32_t magic = dec::rd32(r.f);
    if (magic == dec::kZstdMagic || (magic & 0xfffffff0u) == dec::kSkippableMagic) {
        if (lead)
            put_span(rp, q, 0, p.chunk_bytes);
        if (blockIdx.y != 0 || (p.zfr && p.zfr[2 * q] != 0)) // the parallel path's frame
            return;
        WaveZIo io{ r.f, r.out, lit, lane };
        const uint32_t e = zdec::zstd_decode_frame(io, r.f, len, uint32_t(p.chunk_bytes), s_t);
        if (e != dec::kOk && lane == 0)
            atomicMax(&p.status[q], e);
        return;
    }
    dec::FrameInfo h;
    const uint32_t st = dec::parse_header(r.f, r.len, p.chunk_bytes, h, dec::kCodecZstd);
    if (st != dec::kOk) {
        if (lead)
            atomicMax(&p.status[q], st);
        return;
    }
    if (h.memcpyed) {
        bool diff = false;
        if (lead)
            put_span(rp, q, want.lo, want.hi);
        const uint64_t step = uint64_t(gridDim.y) * kDecodeLdsBytes;
        for (uint64_t b = want.lo + uint64_t(blockIdx.y) * kDecodeLdsBytes; b < want.hi;
             b += step) {
            const uint64_t left = want.hi - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<false>(r.out + b, r.f + 16 + b, n, lane, 64, diff);
        }
        return;
    }
    // want.hi <= chunk_bytes == h.nbytes and want.lo < want.hi: at least one block
    const dec::BlockRange br = dec::blocks_of_range(h, want.lo, want.hi);
    if (lead)
        put_span(rp, q, br.lo, br.hi);
    uint8_t* base = staged<false>(false, h.mode) ? scr : r.out;
    uint32_t err = dec::kOk;
    for (uint32_t j = br.jlo + blockIdx.y; j < br.jhi && err == dec::kOk; j += gridDim.y) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        uint32_t pos = 0;
        err = dec::block_start(r.f, h, j, pos);
        for (uint32_t s = 0; s < bi.ns && err == dec::kOk; ++s) {
            uint32_t src = 0, csz = 0;
            err = dec::next_stream(r.f, h, pos, src, csz);
            if (err != dec::kOk)
                break;
            src = uni(src);
            csz = uni(csz);
            WaveZIo io{ r.f + src, base + uint64_t(j) * h.blocksize + uint64_t(s) * bi.slen, lit,
                        lane };
            if (csz == bi.slen) { // stored raw
                if (bi.slen)
                    io.copy_src(0, 0, bi.slen);
            } else {
                err = zdec::zstd_decode_frame(io, r.f + src, csz, bi.slen, s_t);
            }
        }
    }
    if (err != dec::kOk && lane == 0)
        atomicMax(&p.status[q], err);
}

__global__ void __launch_bounds__(kFinishThreads)
zstd_finish_ranged(RangedParams rp)
{
    const DecodeParams& p = rp.p;
    const uint32_t tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const dec::ByteRange want = rp.ranges[q];
    if (dec::range_status(want, p.chunk_bytes) != dec::kOk)
        return;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0 || dec::frame_family(r.f, r.len) != dec::kFamilyZstd)
        return;
    if (p.status[q] != dec::kOk) // written by zstd_decode_ranged, complete before this kernel
        return;
    if (dec::rd32(r.f) == dec::kZstdMagic) // decoded in place
        return;
    dec::FrameInfo h;
    if (dec::parse_header(r.f, r.len, p.chunk_bytes, h, dec::kCodecZstd) != dec::kOk ||
        h.memcpyed || !staged<false>(false, h.mode))
        return;
    const dec::BlockRange br = dec::blocks_of_range(h, want.lo, want.hi);
    const uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    bool diff = false;
    for (uint32_t j = br.jlo + blockIdx.y; j < br.jhi; j += gridDim.y) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        unshuffle_block<false>(scr + uint64_t(j) * h.blocksize, r.out + uint64_t(j) * h.blocksize,
                               bi.bsize, h.typesize, h.mode, tid, kFinishThreads, diff);
    }
}

} // namespace

hipError_t
launch_zstd_decode_ranged(const RangedParams& rp, uint64_t max_range_bytes, hipStream_t stream)
{
    const DecodeParams& p = rp.p;
    if (p.n_chunks == 0)
        return hipSuccess;
    if (!rp.ranges || p.bad || !p.scratch || !p.zlit || p.zpasses == 0 ||
        p.zpasses > kZstdMaxPasses || p.scratch_pitch < p.chunk_bytes ||
        p.zlit_pitch < zstd_decode_lit_pitch(p.chunk_bytes))
        return hipErrorInvalidValue;
    // a literal slot per (chunk, pass): no more passes than a full run takes
    uint32_t passes = zstd_decode_passes(p.chunk_bytes);
    if (passes > p.zpasses)
        passes = p.zpasses;
    const dim3 grid(p.n_chunks, ranged_passes(p.chunk_bytes, max_range_bytes, passes));
    hipLaunchKernelGGL(zstd_decode_ranged, grid, dim3(64), 0, stream, rp);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(zstd_finish_ranged, grid, dim3(kFinishThreads), 0, stream, rp);
    return hipGetLastError();
}

uint32_t
zstd_decode_passes(uint64_t max_chunk_bytes)
{
    const uint64_t n = (max_chunk_bytes + kDecodeLdsBytes - 1) / kDecodeLdsBytes;
    return n < 1 ? 1u : n > kZstdMaxPasses ? kZstdMaxPasses : uint32_t(n);
}

uint64_t
zstd_decode_lit_pitch(uint64_t max_chunk_bytes)
{
    // a block regenerates at most kBlockMax literals, and no more than the
    // frame decodes to
    const uint64_t n = max_chunk_bytes < zdec::kBlockMax ? max_chunk_bytes : zdec::kBlockMax;
    return (n + 15) & ~uint64_t(15);
}

hipError_t
launch_zstd_decode(const DecodeParams& p, hipStream_t stream)
{
    if (p.n_chunks == 0)
        return hipSuccess;
    if (!p.scratch || !p.zlit || p.zpasses == 0 || p.zpasses > kZstdMaxPasses ||
        p.scratch_pitch < p.chunk_bytes || p.zlit_pitch < zstd_decode_lit_pitch(p.chunk_bytes))
        return hipErrorInvalidValue;
    uint32_t passes = zstd_decode_passes(p.chunk_bytes);
    if (passes > p.zpasses)
        passes = p.zpasses;
    const dim3 grid(p.n_chunks, passes);
    if (p.bad)
        hipLaunchKernelGGL(zstd_decode<true>, grid, dim3(64), 0, stream, p);
    else
        hipLaunchKernelGGL(zstd_decode<false>, grid, dim3(64), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    if (p.bad)
        hipLaunchKernelGGL(zstd_finish<true>, grid, dim3(kFinishThreads), 0, stream, p);
    else
        hipLaunchKernelGGL(zstd_finish<false>, grid, dim3(kFinishThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace aqz
