// aqz_pack.hip -- pitched level-0 frames packed into a contiguous device
// buffer (the packed route of aqz_stage_append_strided, aqz_strided.hh): the
// sources the fused kernels cannot load in place -- a pitch or address that is
// no multiple of 16, XY storage orders, the frames of a 2x2x2 batch that go to
// the generic cascade, non-default tuning.
//
// One item = up to kPackRows rows of one frame, moved by CopyMover (the
// reader's mover, aqz_unsplit_dev.hh): a wave's lanes take consecutive units
// of a row, four units per thread are in flight before the first store, loads
// and stores are nontemporal.  Units are 16, 8, 4, 2 or 1 bytes, chosen per
// launch on the host (strided::pack_unit).  Only bytes inside the rows are
// read: unit u of a row is read iff (u + 1) * V <= row_bytes.  No scratch,
// no LDS.
#include "aqz_engine.hh"
#include "aqz_strided.hh"
#include "aqz_unsplit_dev.hh"

#include <hip/hip_runtime.h>

namespace aqz {

namespace {

constexpr uint32_t kPackRows = 64;

template<int V>
__global__ __launch_bounds__(kThreads) void
pack_frames(const PackParams p)
{
    const uint64_t per_frame = (p.rows + kPackRows - 1) / kPackRows;
    const uint64_t total = per_frame * p.n_frames;
    CopyMover<V> m{ p.src, nullptr, threadIdx.x };
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        const uint64_t fi = it / per_frame;
        const uint32_t y0 = uint32_t(it - fi * per_frame) * kPackRows;
        unsplit::Rect r{};
        r.rows = min(kPackRows, p.rows - y0);
        r.src = uint64_t(y0) * p.row_stride;
        r.src_pitch = p.row_stride;
        r.dst = uint64_t(y0) * p.row_bytes;
        r.dst_pitch = p.row_bytes;
        r.dst_row_bytes = p.row_bytes;
        m.dst = p.dst + fi * (uint64_t(p.rows) * p.row_bytes);
        m.copy(fi * p.frame_stride, r);
    }
}

} // namespace

hipError_t
launch_pack_frames(const PackParams& p, uint32_t unit, hipStream_t stream)
{
    if (p.n_frames == 0 || p.rows == 0 || p.row_bytes == 0)
        return hipSuccess;
    // the mover counts a slab's units in 32 bits; every unit inside a row
    if (p.row_bytes * kPackRows > 0xffffffffull || p.row_stride < p.row_bytes ||
        unit == 0 || p.row_bytes % unit || p.row_stride % unit || p.frame_stride % unit ||
        reinterpret_cast<uintptr_t>(p.src) % unit || reinterpret_cast<uintptr_t>(p.dst) % unit)
        return hipErrorInvalidValue;
    const uint64_t total = uint64_t((p.rows + kPackRows - 1) / kPackRows) * p.n_frames;
    const dim3 grid(uint32_t(total < kMaxGrid ? total : kMaxGrid)), block(kThreads);
    switch (unit) {
        case 16: hipLaunchKernelGGL(pack_frames<16>, grid, block, 0, stream, p); break;
        case 8: hipLaunchKernelGGL(pack_frames<8>, grid, block, 0, stream, p); break;
        case 4: hipLaunchKernelGGL(pack_frames<4>, grid, block, 0, stream, p); break;
        case 2: hipLaunchKernelGGL(pack_frames<2>, grid, block, 0, stream, p); break;
        case 1: hipLaunchKernelGGL(pack_frames<1>, grid, block, 0, stream, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace aqz
