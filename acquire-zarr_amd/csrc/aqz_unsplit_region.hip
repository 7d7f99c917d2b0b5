// aqz_unsplit_region.hip -- the region variants of the un-split kernels
// (aqz_unsplit.hip): the crop of a few frames of a chunk layer, written as a
// strided rectangle.  The address map, the walk over the tiles and slabs that
// meet the region and every bound live in aqz_unsplit.hh, shared with the
// host; the byte movers in aqz_unsplit_dev.hh are those of the whole-frame
// kernels, which this file leaves as they are.
#include "aqz_reader.hh"
#include "aqz_unsplit_dev.hh"

#include <hip/hip_runtime.h>

namespace aqz {

namespace {

// The region variants: the same movers and the same grid-stride walk, over
// the (frame, slab row, tile column) items of a crop (unsplit::region_item).
template<int V>
__global__ __launch_bounds__(kThreads) void
unsplit_region_copy(const unsplit::RegionParams q)
{
    const uint64_t per_frame = unsplit::region_items_per_frame(q.p.g, q.r);
    const uint64_t total = per_frame * q.p.count;
    CopyMover<V> m{ q.p.src, nullptr, threadIdx.x };
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t fi = uint32_t(it / per_frame);
        m.dst = q.p.dst + fi * q.p.dst_stride;
        unsplit::region_item<false>(q.p.g, q.r, q.p.tab_grp, q.p.tab_off, q.p.chunk_src,
                                    q.p.first + fi, it - fi * per_frame, m);
    }
}

template<int BPP, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void
unsplit_region_xy(const unsplit::RegionParams q)
{
    using W = typename Unit<BPP>::type;
    __shared__ W tile[unsplit::kSlabRows][unsplit::kSlabRows + 1];
    const uint64_t per_frame = unsplit::region_items_per_frame(q.p.g, q.r);
    const uint64_t total = per_frame * q.p.count;
    XyMover<BPP, ALIGNED> m{ q.p.src, nullptr, threadIdx.x, tile };
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint32_t fi = uint32_t(it / per_frame);
        m.dst = q.p.dst + fi * q.p.dst_stride;
        unsplit::region_item<true>(q.p.g, q.r, q.p.tab_grp, q.p.tab_off, q.p.chunk_src,
                                   q.p.first + fi, it - fi * per_frame, m);
    }
}

} // namespace

hipError_t
launch_unsplit_region(const unsplit::RegionParams& q, uint64_t align, hipStream_t stream)
{
    const unsplit::Geom& g = q.p.g;
    if (q.p.count == 0)
        return hipSuccess;
    // what the movers' 32-bit unit counts, the map's tables and the crop take
    if (uint64_t(g.tw) * g.bpp * unsplit::kSlabRows > 0xffffffffull ||
        uint64_t(q.p.first) + q.p.count > g.n_frames || !unsplit::region_valid(g, q.r) ||
        q.p.dst_stride < unsplit::region_frame_extent(g, q.r))
        return hipErrorInvalidValue;
    const uint64_t per_frame = unsplit::region_items_per_frame(g, q.r);
    if (per_frame > 0xffffffffull) // total = per_frame * count stays inside 64 bits
        return hipErrorInvalidValue;
    const uint64_t total = per_frame * q.p.count;
    const dim3 grid(uint32_t(total < kMaxGrid ? total : kMaxGrid)), block(kThreads);
    if (!g.xy) {
        switch (unsplit::region_copy_unit(g, q.r, align)) {
            case 16:
                hipLaunchKernelGGL(unsplit_region_copy<16>, grid, block, 0, stream, q);
                break;
            case 8: hipLaunchKernelGGL(unsplit_region_copy<8>, grid, block, 0, stream, q); break;
            case 4: hipLaunchKernelGGL(unsplit_region_copy<4>, grid, block, 0, stream, q); break;
            case 2: hipLaunchKernelGGL(unsplit_region_copy<2>, grid, block, 0, stream, q); break;
            default:
                hipLaunchKernelGGL(unsplit_region_copy<1>, grid, block, 0, stream, q);
                break;
        }
        return hipGetLastError();
    }
    const bool al = unsplit::region_pixel_aligned(g, q.r, align);
#define AQZ_XY(BPP)                                                                            \
    if (al)                                                                                    \
        hipLaunchKernelGGL((unsplit_region_xy<BPP, true>), grid, block, 0, stream, q);         \
    else                                                                                       \
        hipLaunchKernelGGL((unsplit_region_xy<BPP, false>), grid, block, 0, stream, q);        \
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
