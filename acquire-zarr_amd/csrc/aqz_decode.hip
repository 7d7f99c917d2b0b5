// aqz_decode.hip -- blosc1 + LZ4 decoding of frames resident in HBM on
// gfx950 (see aqz_decode.hh; the parse and its bounds: aqz_lz4dec.hh).
//
//   blosc_decode         grid (frame, pass).  A workgroup of 8 waves takes a
//                        group of up to 8 consecutive blocks of its frame
//                        whose decoded bytes fit kDecodeLdsBytes of LDS:
//                        one thread per block walks the block's csize chain
//                        into an LDS stream table, then one wave per stream
//                        decodes it -- the LZ4 token walk is wave-uniform
//                        (control bytes come out of a 256-byte register
//                        window by v_readlane, lengths and positions stay in
//                        SGPRs), the 64 lanes move the literal and match
//                        bytes -- and after a barrier all 512 threads
//                        un-shuffle the blocks from LDS straight into the
//                        destination chunk (or compare them with it).
//                        Compressed bytes are read once, chunk bytes written
//                        once.  Memcpyed and zero-length frames are copied /
//                        zero-filled by the same grid.
//   blosc_unshuffle_big  frames whose block size exceeds the LDS budget
//                        (c-blosc's own: 64 KiB and more) were decoded into
//                        a global scratch slot; this un-shuffles them.
#include "aqz_decode.hh"
#include "aqz_decode_dev.hh"

namespace aqz {
namespace {

constexpr uint32_t kThreads = 512;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kMaxGroup = 8; // blocks per workgroup pass
constexpr uint32_t kMaxStreams = kMaxGroup * dec::kMaxSplit;
constexpr uint32_t kBigThreads = 256;
constexpr uint32_t kMaxPasses = 1024; // grid.y

// The byte movers of one wave for dec::lz4_decode.  kGlobalOut: the output
// is global memory (the scratch slot of a large block), where a lane re-reads
// bytes other lanes of the wave have just stored: a workgroup-scope fence
// separates the stores from the dependent loads.  LDS operations of one wave
// execute in order; there the fence is at wavefront scope (compiler ordering).
template<bool kGlobalOut>
struct WaveIo
{
    const uint8_t* src;
    uint8_t* out;
    uint32_t n_src;
    uint32_t lane;
    uint32_t win;  // bytes [base + 4 * lane, + 4) of the source
    uint32_t base;

    __device__ __forceinline__ WaveIo(const uint8_t* s, uint8_t* o, uint32_t n, uint32_t l)
      : src(s)
      , out(o)
      , n_src(n)
      , lane(l)
    {
        refill(0);
    }

    __device__ __forceinline__ void refill(uint32_t q)
    {
        base = q;
        const uint32_t a = q + 4 * lane;
        uint32_t w = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (a + k < n_src)
                w |= uint32_t(src[a + k]) << (8 * k);
        win = w;
    }

    __device__ __forceinline__ uint32_t ctl(uint32_t q)
    {
        if (q - base >= 256u)
            refill(q);
        const uint32_t r = q - base;
        const uint32_t w = uint32_t(__builtin_amdgcn_readlane(int(win), int(uni(r >> 2))));
        return (w >> (8 * (r & 3u))) & 0xffu;
    }

    __device__ __forceinline__ void sync()
    {
        if (kGlobalOut) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }

    __device__ __forceinline__ void literals(uint32_t d, uint32_t q, uint32_t n)
    {
        const uint8_t* s = src + q;
        uint8_t* o = out + d;
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
        sync();
    }

    // every byte read lies before out + d: written by an earlier call
    __device__ __forceinline__ void match(uint32_t d, uint32_t off, uint32_t n)
    {
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
        sync();
    }
};

// One stream record: stored raw (csize == its length) or an LZ4 block.
template<bool kGlobalOut>
__device__ __forceinline__ uint32_t
decode_stream(const uint8_t* src, uint32_t csize, uint8_t* out, uint32_t slen, uint32_t lane)
{
    WaveIo<kGlobalOut> io(src, out, csize, lane);
    if (csize == slen) {
        if (slen)
            io.literals(0, 0, slen);
        return dec::kOk;
    }
    return dec::lz4_decode(io, csize, slen);
}

template<bool kCompare>
__global__ void __launch_bounds__(kThreads)
blosc_decode(DecodeParams p)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[kDecodeLdsBytes];
    __shared__ uint32_t s_src[kMaxStreams], s_csz[kMaxStreams], s_dst[kMaxStreams],
      s_len[kMaxStreams];
    __shared__ dec::FrameInfo s_h;
    __shared__ uint32_t s_st, s_err_walk, s_err_dec, s_nstreams;

    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);
    const uint32_t q = blockIdx.x;
    const bool lead = blockIdx.y == 0 && tid == 0;
    bool diff = false;
    FrameRef r;
    if (!frame_ref(p, q, r)) {
        if (lead)
            atomicMax(&p.status[q], uint32_t(dec::kBadHeader));
        return;
    }
    const uint64_t span = uint64_t(gridDim.y) * kDecodeLdsBytes;
    if (r.len == 0) { // a skipped chunk reads as fill_value 0
        if (lead)
            atomicMax(&p.status[q], uint32_t(dec::kSkipped));
        for (uint64_t b = uint64_t(blockIdx.y) * kDecodeLdsBytes; b < p.chunk_bytes; b += span) {
            const uint64_t left = p.chunk_bytes - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<kCompare>(r.out + b, nullptr, n, tid, kThreads, diff);
        }
        if (kCompare && diff)
            p.bad[q] = 1;
        return;
    }
    if (p.codecs) {
        const uint32_t fam = dec::frame_family(r.f, r.len);
        if (fam == dec::kFamilyZstd && (p.codecs & dec::kFamilyZstd))
            return; // the zstd kernels' frame
        if (fam == dec::kFamilyLz4 && !(p.codecs & dec::kFamilyLz4)) {
            if (lead)
                atomicMax(&p.status[q], uint32_t(dec::kUnsupported));
            return;
        }
    }
    if (tid == 0) {
        s_st = dec::parse_header(r.f, r.len, p.chunk_bytes, s_h);
        s_err_walk = 0;
        s_err_dec = 0;
    }
    __syncthreads();
    if (s_st != dec::kOk) {
        if (lead)
            atomicMax(&p.status[q], s_st);
        return;
    }
    const dec::FrameInfo h = s_h;
    if (h.memcpyed) {
        for (uint64_t b = uint64_t(blockIdx.y) * kDecodeLdsBytes; b < h.nbytes; b += span) {
            const uint64_t left = h.nbytes - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<kCompare>(r.out + b, r.f + 16 + b, n, tid, kThreads, diff);
        }
        if (kCompare && diff)
            p.bad[q] = 1;
        return;
    }
    const bool big = h.blocksize > kDecodeLdsBytes;
    if (big && (kCompare || !p.scratch)) {
        if (lead)
            atomicMax(&p.status[q], uint32_t(dec::kUnsupported));
        return;
    }
    // blocks of a group sit 16-byte aligned in LDS
    const uint32_t stride = big ? 0u : (h.blocksize + 15u) & ~15u;
    uint32_t gb = big ? 1u : kDecodeLdsBytes / stride;
    if (gb > kMaxGroup)
        gb = kMaxGroup;
    const uint32_t ns_full = dec::block_info(h, 0).ns; // of every block but a leftover one
    uint8_t* scr = big ? p.scratch + uint64_t(q) * p.scratch_pitch : nullptr;
    uint32_t err = 0;

    for (uint32_t g0 = blockIdx.y * gb; g0 < h.nblocks; g0 += gridDim.y * gb) {
        const uint32_t nb = h.nblocks - g0 < gb ? h.nblocks - g0 : gb;
        if (tid < nb) {
            const uint32_t j = g0 + tid;
            const dec::BlockInfo bi = dec::block_info(h, j);
            const uint32_t first = tid * ns_full; // the blocks before j are full
            uint32_t pos = 0;
            uint32_t e = dec::block_start(r.f, h, j, pos);
            for (uint32_t s = 0; s < bi.ns && e == dec::kOk; ++s) {
                uint32_t src = 0, csz = 0;
                e = dec::next_stream(r.f, h, pos, src, csz);
                if (e == dec::kOk) {
                    s_src[first + s] = src;
                    s_csz[first + s] = csz;
                    s_dst[first + s] = (big ? j * h.blocksize : tid * stride) + s * bi.slen;
                    s_len[first + s] = bi.slen;
                }
            }
            if (e != dec::kOk)
                atomicMax(&s_err_walk, e);
            if (tid == nb - 1)
                s_nstreams = first + bi.ns;
        }
        __syncthreads();
        err = s_err_walk;
        if (err)
            break;
        const uint32_t nstr = s_nstreams;
        for (uint32_t k = wave; k < nstr; k += kWaves) {
            const uint32_t src = uni(s_src[k]), csz = uni(s_csz[k]), dof = uni(s_dst[k]),
                           slen = uni(s_len[k]);
            const uint32_t e = big ? decode_stream<true>(r.f + src, csz, scr + dof, slen, lane)
                                   : decode_stream<false>(r.f + src, csz, s_blk + dof, slen, lane);
            if (e != dec::kOk && lane == 0)
                atomicMax(&s_err_dec, e);
        }
        __syncthreads();
        err = s_err_dec;
        if (err)
            break;
        if (!big) {
            for (uint32_t b = 0; b < nb; ++b) {
                const uint32_t j = g0 + b;
                const dec::BlockInfo bi = dec::block_info(h, j);
                unshuffle_block<kCompare>(s_blk + b * stride, r.out + uint64_t(j) * h.blocksize,
                                          bi.bsize, h.typesize, h.mode, tid, kThreads, diff);
            }
            __syncthreads(); // the next pass reuses the LDS
        }
    }
    if (err && tid == 0)
        atomicMax(&p.status[q], err);
    if (kCompare && diff)
        p.bad[q] = 1;
}

__global__ void __launch_bounds__(kBigThreads)
blosc_unshuffle_big(DecodeParams p)
{
    __shared__ dec::FrameInfo s_h;
    __shared__ uint32_t s_st;
    const uint32_t tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0)
        return;
    if (tid == 0)
        s_st = dec::parse_header(r.f, r.len, p.chunk_bytes, s_h);
    __syncthreads();
    if (s_st != dec::kOk)
        return;
    const dec::FrameInfo h = s_h;
    if (h.memcpyed || h.blocksize <= kDecodeLdsBytes || p.status[q] != dec::kOk)
        return;
    const uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    bool diff = false;
    for (uint32_t j = blockIdx.y; j < h.nblocks; j += gridDim.y) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        unshuffle_block<false>(scr + uint64_t(j) * h.blocksize, r.out + uint64_t(j) * h.blocksize,
                               bi.bsize, h.typesize, h.mode, tid, kBigThreads, diff);
    }
}

// ---- ranged decode ----------------------------------------------------------
// blosc_decode and blosc_unshuffle_big over the blocks that meet a byte range
// (aqz_decode.hh, RangedParams).  They are kernels of their own, with the
// group loop restated, so that the code of a full run is what it was.  What
// differs: the range is checked before the frame is looked at, the group walk
// runs over blocks [jlo, jhi) and starts at jlo (workgroup y takes the y-th
// needed group, so the needed groups spread over the first workgroups
// whatever their place in the chunk), copies and zero fills cover [lo, hi),
// and the lead thread reports the span.

__global__ void __launch_bounds__(kThreads)
blosc_decode_ranged(RangedParams rp)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[kDecodeLdsBytes];
    __shared__ uint32_t s_src[kMaxStreams], s_csz[kMaxStreams], s_dst[kMaxStreams],
      s_len[kMaxStreams];
    __shared__ dec::FrameInfo s_h;
    __shared__ uint32_t s_st, s_err_walk, s_err_dec, s_nstreams;

    const DecodeParams& p = rp.p;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = uni(tid >> 6);
    const uint32_t q = blockIdx.x;
    const bool lead = blockIdx.y == 0 && tid == 0;
    bool diff = false; // the emitters' compare word; never set here
    const dec::ByteRange want = rp.ranges[q];
    const uint32_t rs = dec::range_status(want, p.chunk_bytes);
    if (rs != dec::kOk) { // empty or bad, for a frame of any family: not looked at
        if (lead)
            atomicMax(&p.status[q], rs);
        return;
    }
    FrameRef r;
    if (!frame_ref(p, q, r)) {
        if (lead)
            atomicMax(&p.status[q], uint32_t(dec::kBadHeader));
        return;
    }
    const uint64_t step = uint64_t(gridDim.y) * kDecodeLdsBytes;
    if (r.len == 0) { // a skipped chunk reads as fill_value 0
        if (lead) {
            atomicMax(&p.status[q], uint32_t(dec::kSkipped));
            put_span(rp, q, want.lo, want.hi);
        }
        for (uint64_t b = want.lo + uint64_t(blockIdx.y) * kDecodeLdsBytes; b < want.hi;
             b += step) {
            const uint64_t left = want.hi - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<false>(r.out + b, nullptr, n, tid, kThreads, diff);
        }
        return;
    }
    if (p.codecs) {
        const uint32_t fam = dec::frame_family(r.f, r.len);
        if (fam == dec::kFamilyZstd && (p.codecs & dec::kFamilyZstd))
            return; // the zstd kernels' frame
        if (fam == dec::kFamilyLz4 && !(p.codecs & dec::kFamilyLz4)) {
            if (lead)
                atomicMax(&p.status[q], uint32_t(dec::kUnsupported));
            return;
        }
    }
    if (tid == 0) {
        s_st = dec::parse_header(r.f, r.len, p.chunk_bytes, s_h);
        s_err_walk = 0;
        s_err_dec = 0;
    }
    __syncthreads();
    if (s_st != dec::kOk) {
        if (lead)
            atomicMax(&p.status[q], s_st);
        return;
    }
    const dec::FrameInfo h = s_h;
    if (h.memcpyed) {
        if (lead)
            put_span(rp, q, want.lo, want.hi);
        for (uint64_t b = want.lo + uint64_t(blockIdx.y) * kDecodeLdsBytes; b < want.hi;
             b += step) {
            const uint64_t left = want.hi - b;
            const uint32_t n = left < kDecodeLdsBytes ? uint32_t(left) : kDecodeLdsBytes;
            copy_bytes<false>(r.out + b, r.f + 16 + b, n, tid, kThreads, diff);
        }
        return;
    }
    const bool big = h.blocksize > kDecodeLdsBytes;
    if (big && !p.scratch) {
        if (lead)
            atomicMax(&p.status[q], uint32_t(dec::kUnsupported));
        return;
    }
    // want.hi <= chunk_bytes == h.nbytes and want.lo < want.hi: at least one block
    const dec::BlockRange br = dec::blocks_of_range(h, want.lo, want.hi);
    if (lead)
        put_span(rp, q, br.lo, br.hi);
    // blocks of a group sit 16-byte aligned in LDS
    const uint32_t stride = big ? 0u : (h.blocksize + 15u) & ~15u;
    uint32_t gb = big ? 1u : kDecodeLdsBytes / stride;
    if (gb > kMaxGroup)
        gb = kMaxGroup;
    const uint32_t ns_full = dec::block_info(h, 0).ns; // of every block but a leftover one
    uint8_t* scr = big ? p.scratch + uint64_t(q) * p.scratch_pitch : nullptr;
    uint32_t err = 0;

    for (uint32_t g0 = br.jlo + blockIdx.y * gb; g0 < br.jhi; g0 += gridDim.y * gb) {
        const uint32_t nb = br.jhi - g0 < gb ? br.jhi - g0 : gb;
        if (tid < nb) {
            const uint32_t j = g0 + tid;
            const dec::BlockInfo bi = dec::block_info(h, j);
            const uint32_t first = tid * ns_full; // the blocks before j are full
            uint32_t pos = 0;
            uint32_t e = dec::block_start(r.f, h, j, pos);
            for (uint32_t s = 0; s < bi.ns && e == dec::kOk; ++s) {
                uint32_t src = 0, csz = 0;
                e = dec::next_stream(r.f, h, pos, src, csz);
                if (e == dec::kOk) {
                    s_src[first + s] = src;
                    s_csz[first + s] = csz;
                    s_dst[first + s] = (big ? j * h.blocksize : tid * stride) + s * bi.slen;
                    s_len[first + s] = bi.slen;
                }
            }
            if (e != dec::kOk)
                atomicMax(&s_err_walk, e);
            if (tid == nb - 1)
                s_nstreams = first + bi.ns;
        }
        __syncthreads();
        err = s_err_walk;
        if (err)
            break;
        const uint32_t nstr = s_nstreams;
        for (uint32_t k = wave; k < nstr; k += kWaves) {
            const uint32_t src = uni(s_src[k]), csz = uni(s_csz[k]), dof = uni(s_dst[k]),
                           slen = uni(s_len[k]);
            const uint32_t e = big ? decode_stream<true>(r.f + src, csz, scr + dof, slen, lane)
                                   : decode_stream<false>(r.f + src, csz, s_blk + dof, slen, lane);
            if (e != dec::kOk && lane == 0)
                atomicMax(&s_err_dec, e);
        }
        __syncthreads();
        err = s_err_dec;
        if (err)
            break;
        if (!big) {
            for (uint32_t b = 0; b < nb; ++b) {
                const uint32_t j = g0 + b;
                const dec::BlockInfo bi = dec::block_info(h, j);
                unshuffle_block<false>(s_blk + b * stride, r.out + uint64_t(j) * h.blocksize,
                                       bi.bsize, h.typesize, h.mode, tid, kThreads, diff);
            }
            __syncthreads(); // the next pass reuses the LDS
        }
    }
    if (err && tid == 0)
        atomicMax(&p.status[q], err);
}

__global__ void __launch_bounds__(kBigThreads)
blosc_unshuffle_big_ranged(RangedParams rp)
{
    __shared__ dec::FrameInfo s_h;
    __shared__ uint32_t s_st;
    const DecodeParams& p = rp.p;
    const uint32_t tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const dec::ByteRange want = rp.ranges[q];
    if (dec::range_status(want, p.chunk_bytes) != dec::kOk)
        return;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0)
        return;
    if (tid == 0)
        s_st = dec::parse_header(r.f, r.len, p.chunk_bytes, s_h);
    __syncthreads();
    if (s_st != dec::kOk)
        return;
    const dec::FrameInfo h = s_h;
    if (h.memcpyed || h.blocksize <= kDecodeLdsBytes || p.status[q] != dec::kOk)
        return;
    const dec::BlockRange br = dec::blocks_of_range(h, want.lo, want.hi);
    const uint8_t* scr = p.scratch + uint64_t(q) * p.scratch_pitch;
    bool diff = false;
    for (uint32_t j = br.jlo + blockIdx.y; j < br.jhi; j += gridDim.y) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        unshuffle_block<false>(scr + uint64_t(j) * h.blocksize, r.out + uint64_t(j) * h.blocksize,
                               bi.bsize, h.typesize, h.mode, tid, kBigThreads, diff);
    }
}

} // namespace

hipError_t
launch_blosc_decode_ranged(const RangedParams& rp, uint64_t max_range_bytes, hipStream_t stream)
{
    const DecodeParams& p = rp.p;
    if (p.n_chunks == 0)
        return hipSuccess;
    if (!rp.ranges || p.bad)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p.status, 0, size_t(p.n_chunks) * 4, stream);
    if (e != hipSuccess)
        return e;
    if (rp.spans) {
        e = hipMemsetAsync(rp.spans, 0, size_t(p.n_chunks) * sizeof(dec::ByteRange), stream);
        if (e != hipSuccess)
            return e;
    }
    const dim3 grid(p.n_chunks, ranged_passes(p.chunk_bytes, max_range_bytes, kMaxPasses));
    hipLaunchKernelGGL(blosc_decode_ranged, grid, dim3(kThreads), 0, stream, rp);
    e = hipGetLastError();
    if (e != hipSuccess || !p.scratch)
        return e;
    hipLaunchKernelGGL(blosc_unshuffle_big_ranged, grid, dim3(kBigThreads), 0, stream, rp);
    return hipGetLastError();
}

hipError_t
launch_blosc_decode(const DecodeParams& p, hipStream_t stream)
{
    if (p.n_chunks == 0)
        return hipSuccess;
    hipError_t e = hipMemsetAsync(p.status, 0, size_t(p.n_chunks) * 4, stream);
    if (e != hipSuccess)
        return e;
    if (p.bad) {
        e = hipMemsetAsync(p.bad, 0, size_t(p.n_chunks) * 4, stream);
        if (e != hipSuccess)
            return e;
    }
    uint64_t passes = (p.chunk_bytes + kDecodeLdsBytes - 1) / kDecodeLdsBytes;
    if (passes < 1)
        passes = 1;
    if (passes > kMaxPasses)
        passes = kMaxPasses;
    const dim3 grid(p.n_chunks, uint32_t(passes));
    if (p.bad)
        hipLaunchKernelGGL(blosc_decode<true>, grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL(blosc_decode<false>, grid, dim3(kThreads), 0, stream, p);
    e = hipGetLastError();
    if (e != hipSuccess || p.bad || !p.scratch)
        return e;
    hipLaunchKernelGGL(blosc_unshuffle_big, grid, dim3(kBigThreads), 0, stream, p);
    return hipGetLastError();
}

} // namespace aqz
