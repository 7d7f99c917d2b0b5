// strided_sanitize.cpp -- the host side of pitched appends (csrc/aqz_strided.hh,
// CopyPool::copy_rows of csrc/aqz_copy.cpp) run under ASan + UBSan:
//
//   copy_rows
//     for 4 element sizes, the pitches W*bpp, +bpp and +16, three frame
//     strides and pools of 1 and 8 workers (pieces small enough that every
//     worker gets rows): the source canvas is a heap block that ends exactly
//     at the last byte of the last frame's last row, the destination is
//     exactly the packed size, and the result must equal a naive loop.  A read
//     of one byte past a row at the end of the canvas, or a write past the
//     packed frames, is an ASan report.
//
//   strided::refusal
//     every refusal of aqz_stage_append_strided, and the nearest accepted
//     arguments next to each.
//
//   strided::plan_device_batch, pack_unit, contiguous
//     the route of a device batch for every combination of alignment, XY
//     storage order, 2-D / 2x2x2 stage, group-aligned or not, pending plane,
//     tuning.
#include "aqz_copy.hh"
#include "aqz_strided.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace aqz;

namespace {

int failures = 0;

#define CHECK(cond)                                                                            \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                      \
            ++failures;                                                                        \
        }                                                                                      \
    } while (0)

uint32_t
copy_cases()
{
    uint32_t n_cases = 0;
    const size_t W = 37, H = 11, N = 5; // odd on purpose
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    for (const unsigned workers : { 1u, 8u }) {
        CopyPool pool(workers);
        for (const size_t bpp : { size_t(1), size_t(2), size_t(4), size_t(8) }) {
            const size_t rb = W * bpp;
            for (const size_t pitch : { rb, rb + bpp, rb + 16 }) {
                const size_t extent = (H - 1) * pitch + rb;
                for (const size_t fs : { extent, H * pitch, H * pitch + 3 * bpp }) {
                    // the canvas ends at the last byte of the last row
                    const size_t canvas = (N - 1) * fs + extent;
                    std::unique_ptr<uint8_t[]> src(new uint8_t[canvas]);
                    for (size_t i = 0; i < canvas; ++i) {
                        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
                        src[i] = uint8_t(seed >> 56);
                    }
                    std::unique_ptr<uint8_t[]> dst(new uint8_t[N * H * rb]);
                    std::unique_ptr<uint8_t[]> ref(new uint8_t[N * H * rb]);
                    for (size_t k = 0; k < N; ++k)
                        for (size_t y = 0; y < H; ++y)
                            for (size_t x = 0; x < rb; ++x)
                                ref[(k * H + y) * rb + x] = src[k * fs + y * pitch + x];
                    std::memset(dst.get(), 0xA5, N * H * rb);
                    // min_piece of 64 bytes: every worker takes rows
                    pool.copy_rows(dst.get(), src.get(), N, H, rb, pitch, fs, 64);
                    CHECK(std::memcmp(dst.get(), ref.get(), N * H * rb) == 0);
                    // the default piece size: the calling thread alone
                    std::memset(dst.get(), 0x5A, N * H * rb);
                    pool.copy_rows(dst.get(), src.get(), N, H, rb, pitch, fs);
                    CHECK(std::memcmp(dst.get(), ref.get(), N * H * rb) == 0);
                    // a plain copy after a row copy still copies bytes
                    std::memset(dst.get(), 0, rb);
                    pool.copy(dst.get(), src.get(), rb);
                    CHECK(std::memcmp(dst.get(), src.get(), rb) == 0);
                    ++n_cases;
                }
            }
        }
        // nothing to do: no access at all
        pool.copy_rows(nullptr, nullptr, 0, H, 16, 16, 16 * H);
        pool.copy_rows(nullptr, nullptr, N, 0, 16, 16, 0);
    }
    return n_cases;
}

uint32_t
refusal_cases()
{
    using strided::refusal;
    uint32_t n = 0;
    for (const uint64_t bpp : { 1u, 2u, 4u, 8u }) {
        const strided::Shape s{ 100, 30, bpp };
        const uint64_t rb = 100 * bpp, addr = 4096;
        const uint64_t pitch = rb + 16, ext = 29 * pitch + rb;
        CHECK(refusal(s, addr, 3, rb, rb * 30, false) == nullptr); // contiguous
        CHECK(refusal(s, addr, 3, pitch, ext, false) == nullptr);  // tight frame stride
        CHECK(refusal(s, addr, 3, pitch, 30 * pitch, false) == nullptr);
        CHECK(refusal(s, addr + bpp, 3, rb + bpp, ext, false) == nullptr);
        n += 4;
        CHECK(refusal(s, addr, 3, rb - bpp, ext, false) != nullptr); // row_stride < W*bpp
        CHECK(refusal(s, addr, 3, 0, ext, false) != nullptr);
        CHECK(refusal(s, addr, 3, pitch, ext - bpp, false) != nullptr); // frame_stride short
        CHECK(refusal(s, addr, 3, pitch, 0, false) != nullptr);
        CHECK(refusal(s, addr, 3, pitch, ext, true) != nullptr); // level0_split_on_host
        n += 5;
        if (bpp > 1) {
            CHECK(refusal(s, addr, 3, pitch + 1, 64 * (pitch + 16), false) !=
                  nullptr);                                               // row_stride % bpp
            CHECK(refusal(s, addr, 3, pitch + bpp, 64 * (pitch + 16), false) == nullptr);
            CHECK(refusal(s, addr, 3, pitch, 30 * pitch + 1, false) != nullptr); // frame % bpp
            CHECK(refusal(s, addr + 1, 3, pitch, 30 * pitch, false) != nullptr); // address
            n += 4;
        }
        // n_frames * frame_stride overflowing 64 bits; one frame less does not
        const uint64_t big = (uint64_t(1) << 62);
        CHECK(refusal(s, addr, 4, pitch, big, false) != nullptr);
        CHECK(refusal(s, addr, 3, pitch, big, false) == nullptr);
        CHECK(refusal(s, addr, ~uint64_t(0), pitch, 30 * pitch, false) != nullptr);
        // (H - 1) * row_stride overflowing
        CHECK(refusal(s, addr, 1, big, ~uint64_t(0) - (~uint64_t(0) % bpp), false) != nullptr);
        n += 4;
    }
    // a single row: frame_stride may be as small as the row
    const strided::Shape one{ 64, 1, 2 };
    CHECK(strided::refusal(one, 0x1000, 9, 128, 128, false) == nullptr);
    CHECK(strided::refusal(one, 0x1000, 9, 128, 126, false) != nullptr);
    CHECK(strided::contiguous(one, 128, 128));
    CHECK(!strided::contiguous(one, 130, 130));
    const strided::Shape two{ 64, 2, 2 };
    CHECK(strided::contiguous(two, 128, 256));
    CHECK(!strided::contiguous(two, 128, 258)); // a frame stride alone makes it pitched
    return n + 6;
}

uint32_t
plan_cases()
{
    using strided::DevicePlan;
    using strided::plan_device_batch;
    using strided::StageKind;
    uint32_t n = 0;
    const uint64_t base = 0x7f0000001000ull;
    for (int xy = 0; xy < 2; ++xy)
        for (int kind = 0; kind < 3; ++kind) // 0: 2-D, 1: 2x2x2 with a pitched kernel, 2: neither
            for (int tuned = 0; tuned < 2; ++tuned)
                for (int mis = 0; mis < 5; ++mis) // what is misaligned
                    for (const uint64_t written : { 0u, 4u, 3u, 11u })
                        for (int pending = 0; pending < 2; ++pending)
                            for (const uint32_t b : { 1u, 3u, 4u, 8u, 11u }) {
                                StageKind k;
                                k.xy = xy != 0;
                                k.fused_2d = kind == 0;
                                k.pitched_3d = kind == 1;
                                k.group = kind == 0 ? 1 : 4;
                                k.default_tuning = !tuned;
                                const uint64_t addr = base + (mis == 1 ? 8 : 0);
                                const uint64_t row =
                                  mis == 4 ? (uint64_t(1) << 32) : 1120 + (mis == 2 ? 2 : 0);
                                const uint64_t frame = 300 * row + (mis == 3 ? 4 : 0);
                                const DevicePlan p = plan_device_batch(k, addr, row, frame, b,
                                                                       written, pending != 0);
                                CHECK(p.direct + p.packed == b);
                                uint32_t want = 0;
                                if (!xy && !tuned && mis == 0) {
                                    if (kind == 0)
                                        want = b;
                                    else if (kind == 1 && !pending && written % 4 == 0)
                                        want = b / 4 * 4;
                                }
                                CHECK(p.direct == want);
                                ++n;
                            }
    // the pack unit: the largest power of two <= 16 dividing everything
    const strided::Shape s{ 1072, 203, 1 };
    CHECK(strided::pack_unit(s, base, 1120, 232960) == 16);
    CHECK(strided::pack_unit(s, base + 1, 1073, 205 * 1073) == 1);
    CHECK(strided::pack_unit(strided::Shape{ 536, 203, 2 }, base + 2, 1074, 205 * 1074) == 2);
    CHECK(strided::pack_unit(strided::Shape{ 268, 203, 4 }, base + 4, 1076, 205 * 1076) == 4);
    CHECK(strided::pack_unit(strided::Shape{ 134, 203, 8 }, base + 8, 1080, 205 * 1080) == 8);
    CHECK(strided::pack_unit(strided::Shape{ 100, 4, 1 }, base, 1120, 232960) == 4); // row length
    CHECK(strided::host_route(true) == strided::kHostPinned);
    CHECK(strided::host_route(false) == strided::kHostPageable);
    return n + 8;
}

} // namespace

int
main()
{
    const uint32_t c = copy_cases();
    const uint32_t r = refusal_cases();
    const uint32_t p = plan_cases();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("clean: %u copies, %u refusal cases, %u plan cases\n", c, r, p);
    return 0;
}
