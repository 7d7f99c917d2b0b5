// aqz_strided.hh -- pitched level-0 sources (aqz_stage_append_strided): the
// argument checks and the route every batch takes.  Pure host logic with no
// HIP in it: Stage::append_strided runs it, and so does the sanitizer
// program tests/sanitize/strided_sanitize.cpp.
//
// A pitched source is n frames of H rows of W pixels of bpp bytes: row y of
// frame k starts at base + k * frame_stride + y * row_stride.  W and H are
// those of the frames as appended (for an XY-swapped storage order: the
// acquisition rows).  Only the W * bpp bytes of each row are ever read.
#pragma once

#include <cstdint>

namespace aqz {
namespace strided {

struct Shape
{
    uint64_t W, H, bpp; // pixels per row, rows, bytes per pixel (a power of 2)
};

inline uint64_t
row_bytes(const Shape& s)
{
    return s.W * s.bpp;
}

// strides of the same pixels packed contiguously
inline bool
contiguous(const Shape& s, uint64_t row_stride, uint64_t frame_stride)
{
    return row_stride == row_bytes(s) && frame_stride == row_bytes(s) * s.H;
}

// nullptr when the arguments describe a source the stage accepts, else why
// not (the text of aqz_last_error).  Nothing may be enqueued on a refusal.
inline const char*
refusal(const Shape& s, uint64_t addr, uint64_t n_frames, uint64_t row_stride,
        uint64_t frame_stride, bool level0_on_host)
{
    if (level0_on_host)
        return "append_strided: a level0_split_on_host stage takes contiguous frames only";
    if (s.W == 0 || s.H == 0 || s.bpp == 0)
        return "append_strided: empty frames";
    if (row_stride < row_bytes(s))
        return "append_strided: row_stride is smaller than a row (W * bytes per pixel)";
    if (row_stride % s.bpp || frame_stride % s.bpp || addr % s.bpp)
        return "append_strided: the address and both strides must be multiples of the "
               "pixel size";
    // (H - 1) * row_stride + W * bpp, the extent of one frame's rectangle
    uint64_t extent = 0;
    if (__builtin_mul_overflow(s.H - 1, row_stride, &extent) ||
        __builtin_add_overflow(extent, row_bytes(s), &extent))
        return "append_strided: (H - 1) * row_stride + W * bpp overflows 64 bits";
    if (frame_stride < extent)
        return "append_strided: frame_stride is smaller than a frame's rows "
               "((H - 1) * row_stride + W * bytes per pixel)";
    uint64_t total = 0;
    if (__builtin_mul_overflow(n_frames, frame_stride, &total))
        return "append_strided: n_frames * frame_stride overflows 64 bits";
    return nullptr;
}

// What of a stage decides the route of a device-resident batch.
struct StageKind
{
    bool xy = false;             // XY-swapped storage order
    bool fused_2d = false;       // the 2-D fused path (strip / fused_pyramid + edge)
    bool pitched_3d = false;     // 2x2x2 stage whose fused kernel has a pitched variant
    uint32_t group = 1;          // level-0 planes per z group of a 2x2x2 stage
    bool default_tuning = false; // knobs == 0 and the shipped nontemporal policy
};

enum Route : uint32_t
{
    kContiguous = 0,   // exactly Stage::append
    kHostPageable = 1, // copy_rows into the pinned staging buffer, then the H2D
    kHostPinned = 2,   // 2-D DMA straight from the caller's rows
    kDirect = 3,       // device: the fused kernels load the pitched rows
    kPacked = 4,       // device: pack_frames into a contiguous buffer first
};

// may the fused kernels' 16-byte loads read this source as it lies?  (They
// take the row stride as 32 bits, FusedParams::src_row_stride.)
inline bool
direct_aligned(uint64_t addr, uint64_t row_stride, uint64_t frame_stride)
{
    return ((addr | row_stride | frame_stride) & 15u) == 0 && row_stride <= 0xffffffffull;
}

// Frames of one device batch by route: the first `direct` frames are read
// in place, the `packed` ones after them are packed first.
struct DevicePlan
{
    uint32_t direct = 0, packed = 0;
};

// frames_written: level-0 frames written before the batch; pending: the
// generic 2x2x2 cascade holds an unpaired plane (Stage::run_batch sends such
// a batch to the generic cascade whole).
inline DevicePlan
plan_device_batch(const StageKind& k, uint64_t addr, uint64_t row_stride,
                  uint64_t frame_stride, uint32_t n, uint64_t frames_written, bool pending)
{
    DevicePlan p;
    p.packed = n;
    if (k.xy || !k.default_tuning || !direct_aligned(addr, row_stride, frame_stride))
        return p;
    if (k.fused_2d) {
        p.direct = n;
    } else if (k.pitched_3d && k.group > 0 && !pending && frames_written % k.group == 0) {
        p.direct = n / k.group * k.group; // whole z groups (run_batch's n3)
    }
    p.packed = n - p.direct;
    return p;
}

// host sources: a pinned one is DMA'd from where it lies
inline Route
host_route(bool pinned)
{
    return pinned ? kHostPinned : kHostPageable;
}

// Bytes per unit of the pack kernel: the largest power of two <= 16 dividing
// the address, both strides and the row length (as unsplit::copy_unit).
inline uint32_t
pack_unit(const Shape& s, uint64_t addr, uint64_t row_stride, uint64_t frame_stride)
{
    const uint64_t a = addr | row_stride | frame_stride | row_bytes(s) | 16u;
    return uint32_t(a & (~a + 1));
}

} // namespace strided
} // namespace aqz
