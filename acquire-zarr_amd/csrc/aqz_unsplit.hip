// aqz_unsplit.hip -- the device reader's un-split kernels: the chunks of one
// chunk layer back to row-major frames, the inverse of the fused kernels'
// tile stores (Array::write_frame_to_chunks_, array.cpp:537-619) and, for the
// XY-transposed storage order, of load_region_xy / transpose_frame
// (array.cpp:488-534).  The address map and every bound live in
// aqz_unsplit.hh, shared with the host; the byte movers are in
// aqz_unsplit_dev.hh, shared with the region kernels (aqz_unsplit_region.hip).
//
// One launch walks (frame, tile, 64-row slab) items with a grid stride.  Each
// chunk byte is read once and each frame byte written once; nothing goes
// through global memory in between.  Bytes move in units of V = 16, 8, 4, 2
// or 1 bytes, chosen per launch on the host (unsplit::copy_unit) -- 16 when
// tile rows, frame rows, chunk starts and frame starts are all 16-byte
// multiples.  The XY variant moves pixels through a padded 64 x 64 LDS tile
// so that both the chunk reads and the frame writes are row-contiguous.
#include "aqz_reader.hh"
#include "aqz_unsplit_dev.hh"

#include <hip/hip_runtime.h>

namespace aqz {

namespace {

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
