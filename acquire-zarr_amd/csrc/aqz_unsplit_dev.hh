// aqz_unsplit_dev.hh -- the byte movers of the un-split kernels, shared by
// aqz_unsplit.hip (whole frames) and aqz_unsplit_region.hip (crops): the map
// in aqz_unsplit.hh hands them rectangles that lie inside the source chunk
// and the destination.  Device code only.
#pragma once

#include "aqz_unsplit.hh"

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

} // namespace
} // namespace aqz
