// aqz_unsplit.hip -- the device reader's un-split kernels: the chunks of one
// chunk layer back to row-major frames, the inverse of the fused kernels'
// tile stores (Array::write_frame_to_chunks_, array.cpp:537-619) and, for the
// XY-transposed storage order, of load_region_xy / transpose_frame
// (array.cpp:488-534).  The address map and every bound live in
// aqz_unsplit.hh, shared with the host; this file adds only the byte movers.
//
// One launch walks (frame, tile, 64-row slab) items with a grid stride.  Each
// chunk byte is read once and each frame byte written once; nothing goes
// through global memory in between.  Bytes move in units of V = 16, 8, 4, 2
// or 1 bytes, chosen per launch on the host (unsplit::copy_unit) -- 16 when
// tile rows, frame rows, chunk starts and frame starts are all 16-byte
// multiples.  The XY variant moves pixels through a padded 64 x 64 LDS tile
// so that both the chunk reads and the frame writes are row-contiguous.
#include "aqz_reader.hh"

#include <hip/hip_runtime.h>

namespace aqz {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxGrid = 2048; // 8 workgroups per CU; the rest by grid stride

template<typename V>
using gptr = __attribute__((address_space(1))) V*;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

template<int BYTES>
struct Unit;
template<>
struct Unit<16>
{
    using type = u32x4;
};
template<>
struct Unit<8>
{
    using type = u32x2;
};
template<>
struct Unit<4>
{
    using type = uint32_t;
};
template<>
struct Unit<2>
{
    using type = uint16_t;
};
template<>
struct Unit<1>
{
    using type = uint8_t;
};

// streaming accesses: every byte is touched once
template<typename V>
__device__ __forceinline__ V
gload(const uint8_t* p)
{
    return __builtin_nontemporal_load((const gptr<V>)(p));
}

template<typename V>
__device__ __forceinline__ void
gstore(uint8_t* p, V v)
{
    __builtin_nontemporal_store(v, (gptr<V>)(p));
}

// a pixel of BPP bytes that may start at any address
template<int BPP>
struct Bytes
{
    uint8_t b[BPP];
};

template<int BPP, bool ALIGNED>
__device__ __forceinline__ typename Unit<BPP>::type
load_px(const uint8_t* p)
{
    using W = typename Unit<BPP>::type;
    if constexpr (ALIGNED) {
        return gload<W>(p);
    } else {
        union
        {
            W w;
            Bytes<BPP> s;
        } u;
#pragma unroll
        for (int k = 0; k < BPP; ++k)
            u.s.b[k] = *(const gptr<uint8_t>)(p + k);
        return u.w;
    }
}

template<int BPP, bool ALIGNED>
__device__ __forceinline__ void
store_px(uint8_t* p, typename Unit<BPP>::type w)
{
    using W = typename Unit<BPP>::type;
    if constexpr (ALIGNED) {
        gstore<W>(p, w);
    } else {
        union
        {
            W w;
            Bytes<BPP> s;
        } u;
        u.w = w;
#pragma unroll
        for (int k = 0; k < BPP; ++k)
            *(gptr<uint8_t>)(p + k) = u.s.b[k];
    }
}

// Rectangles of units of V bytes, spread over the workgroup row-major: a
// wave's 64 lanes take consecutive units of a row (1 KiB per instruction at
// V = 16).  Four units per thread are in flight before the first store.
template<int V>
struct CopyMover
{
    using U = typename Unit<V>::type;
    const uint8_t* src;
    uint8_t* dst;
    uint32_t tid;

    __device__ void copy(uint64_t base, const unsplit::Rect& r) const
    {
        const uint32_t upr = uint32_t(r.dst_row_bytes / V);
        const uint32_t n = upr * r.rows;
        const uint8_t* s = src + base + r.src;
        uint8_t* d = dst + r.dst;
        for (uint32_t i0 = tid; i0 < n; i0 += 4 * kThreads) {
            U v[4];
            uint64_t at[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t i = i0 + k * kThreads;
                if (i < n) {
                    const uint32_t row = i / upr, u = i - row * upr;
                    v[k] = gload<U>(s + row * r.src_pitch + uint64_t(u) * V);
                    at[k] = row * r.dst_pitch + uint64_t(u) * V;
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (i0 + k * kThreads < n)
                    gstore<U>(d + at[k], v[k]);
        }
    }

    __device__ void zero(const unsplit::Rect& r) const
    {
        const uint32_t upr = uint32_t(r.dst_row_bytes / V);
        const uint32_t n = upr * r.dst_rows;
        uint8_t* d = dst + r.dst;
        for (uint32_t i = tid; i < n; i += kThreads) {
            const uint32_t row = i / upr, u = i - row * upr;
            gstore<U>(d + row * r.dst_pitch + uint64_t(u) * V, U{});
        }
    }
};

// Rectangles of pixels of BPP bytes through a 64 x 64 LDS tile, one column of
// padding against bank conflicts (as load_region_xy pads the forward
// direction): rows of the chunk are read along x, rows of the frame written
// along y.
template<int BPP, bool ALIGNED>
struct XyMover
{
    using W = typename Unit<BPP>::type;
    const uint8_t* src;
    uint8_t* dst;
    uint32_t tid;
    W (*tile)[unsplit::kSlabRows + 1];

    __device__ void transpose(uint64_t base, const unsplit::Rect& r) const
    {
        constexpr uint32_t E = unsplit::kSlabRows;
        const uint32_t lane = tid & (E - 1), q = tid / E; // q < kThreads / E
        const uint8_t* s = src + base + r.src;
        uint8_t* d = dst + r.dst;
        for (uint32_t c0 = 0; c0 < r.cols; c0 += E) {
#pragma unroll 4
            for (uint32_t row = q; row < E; row += kThreads / E) {
                const uint32_t c = c0 + lane;
                if (row < r.rows && c < r.cols)
                    tile[row][lane] =
                      load_px<BPP, ALIGNED>(s + row * r.src_pitch + uint64_t(c) * BPP);
            }
            __syncthreads();
#pragma unroll 4
            for (uint32_t col = q; col < E; col += kThreads / E) {
                const uint32_t c = c0 + col; // storage column = destination row
                if (c < r.cols && lane < r.rows)
                    store_px<BPP, ALIGNED>(d + c * r.dst_pitch + uint64_t(lane) * BPP,
                                           tile[lane][col]);
            }
            __syncthreads();
        }
    }

    __device__ void zero(const unsplit::Rect& r) const
    {
        const uint32_t ppr = uint32_t(r.dst_row_bytes / BPP);
        const uint32_t n = ppr * r.dst_rows;
        uint8_t* d = dst + r.dst;
        for (uint32_t i = tid; i < n; i += kThreads) {
            const uint32_t row = i / ppr, u = i - row * ppr;
            store_px<BPP, ALIGNED>(d + row * r.dst_pitch + uint64_t(u) * BPP, W{});
        }
    }
};

template<int V>
__global__ __launch_bounds__(kThreads) void
unsplit_copy(const unsplit::Params p)
{
    const uint64_t per_frame = unsplit::items_per_frame(p.g);
    const uint64_t total = per_frame * p.count;
    CopyMover<V> m{ p.src, nullptr, threadIdx.x };
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t fi = uint32_t(it / per_frame);
        m.dst = p.dst + fi * p.dst_stride;
        unsplit::unsplit_item<false>(p.g, p.tab_grp, p.tab_off, p.chunk_src, p.first + fi,
                                     it - fi * per_frame, m);
    }
}

template<int BPP, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void
unsplit_xy(const unsplit::Params p)
{
    using W = typename Unit<BPP>::type;
    __shared__ W tile[unsplit::kSlabRows][unsplit::kSlabRows + 1];
    const uint64_t per_frame = unsplit::items_per_frame(p.g);
    const uint64_t total = per_frame * p.count;
    XyMover<BPP, ALIGNED> m{ p.src, nullptr, threadIdx.x, tile };
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t fi = uint32_t(it / per_frame);
        m.dst = p.dst + fi * p.dst_stride;
        unsplit::unsplit_item<true>(p.g, p.tab_grp, p.tab_off, p.chunk_src, p.first + fi,
                                    it - fi * per_frame, m);
    }
}

// chunk_src of decoded chunks lying at a pitch: chunk c at c * pitch, or
// never written when its has_data word is not the layer's tag
__global__ void
unsplit_chunk_table(uint64_t* chunk_src, uint32_t n, uint64_t pitch, const uint32_t* has_data,
                    uint32_t tag)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n)
        chunk_src[c] = (!has_data || has_data[c] == tag) ? c * pitch : unsplit::kNoChunk;
}

} // namespace

hipError_t
launch_chunk_table(uint64_t* chunk_src, uint32_t n, uint64_t pitch, const uint32_t* has_data,
                   uint32_t tag, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(unsplit_chunk_table, dim3((n + 255) / 256), dim3(256), 0, stream,
                       chunk_src, n, pitch, has_data, tag);
    return hipGetLastError();
}

hipError_t
launch_unsplit(const unsplit::Params& p, uint64_t align, hipStream_t stream)
{
    const unsplit::Geom& g = p.g;
    if (p.count == 0)
        return hipSuccess;
    // what the movers' 32-bit unit counts and the map's tables take
    if (uint64_t(g.tw) * g.bpp * unsplit::kSlabRows > 0xffffffffull ||
        uint64_t(p.first) + p.count > g.n_frames || p.dst_stride < unsplit::frame_bytes(g))
        return hipErrorInvalidValue;
    const uint64_t total = unsplit::items_per_frame(g) * p.count;
    const dim3 grid(uint32_t(total < kMaxGrid ? total : kMaxGrid)), block(kThreads);
    if (!g.xy) {
        switch (unsplit::copy_unit(g, align)) {
            case 16: hipLaunchKernelGGL(unsplit_copy<16>, grid, block, 0, stream, p); break;
            case 8: hipLaunchKernelGGL(unsplit_copy<8>, grid, block, 0, stream, p); break;
            case 4: hipLaunchKernelGGL(unsplit_copy<4>, grid, block, 0, stream, p); break;
            case 2: hipLaunchKernelGGL(unsplit_copy<2>, grid, block, 0, stream, p); break;
            default: hipLaunchKernelGGL(unsplit_copy<1>, grid, block, 0, stream, p); break;
        }
        return hipGetLastError();
    }
    const bool al = unsplit::pixel_aligned(g, align);
#define AQZ_XY(BPP)                                                                            \
    if (al)                                                                                    \
        hipLaunchKernelGGL((unsplit_xy<BPP, true>), grid, block, 0, stream, p);                \
    else                                                                                       \
        hipLaunchKernelGGL((unsplit_xy<BPP, false>), grid, block, 0, stream, p);               \
    break;
    switch (g.bpp) {
        case 1: AQZ_XY(1)
        case 2: AQZ_XY(2)
        case 4: AQZ_XY(4)
        case 8: AQZ_XY(8)
        default: return hipErrorInvalidValue;
    }
#undef AQZ_XY
    return hipGetLastError();
}

} // namespace aqz
