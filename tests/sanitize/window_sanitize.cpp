// window_sanitize.cpp -- the range math of a window load run on the host
// under ASan + UBSan:
//
//   region_chunk_ranges (csrc/aqz_region.cpp, over unsplit::region_hull_frame)
//     for the geometries of region_sanitize.cpp and each element size, every
//     region of its list and three frame ranges: the hull of every chunk must
//     be the first and one past the last byte of the crop's pixels in it,
//     found pixel by pixel, and the chunks must be region_chunks's.
//
//   dec::blocks_of_range and dec::range_status (csrc/aqz_lz4dec.hh)
//     for seeded random blosc1 headers -- parsed by dec::parse_header out of a
//     heap block of exactly the header and the block table -- with block sizes
//     above nbytes, with and without a leftover block, and ranges that are
//     empty, reversed, end at nbytes or lie past it: the blocks must be those
//     whose bytes meet the range, found block by block, and the span theirs.
#include "aqz_geometry.hh"
#include "aqz_lz4dec.hh"
#include "aqz_region.hh"
#include "aqz_unsplit.hh"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace aqz;

namespace {

struct Case
{
    const char* name;
    std::vector<Dim> dims;
    std::vector<size_t> order;
};

uint32_t
odd_below(uint32_t v) // the largest odd number below v, 1 at the least
{
    if (v < 3)
        return 1;
    return (v - 1) % 2 ? v - 1 : v - 2;
}

// the regions of region_sanitize.cpp
std::vector<RegionArg>
regions_of(const unsplit::Geom& g)
{
    const uint32_t Wa = g.xy ? g.H : g.W, Ha = g.xy ? g.W : g.H;
    const uint32_t twa = g.xy ? g.th : g.tw, tha = g.xy ? g.tw : g.th;
    const uint32_t ntxa = parts_along(Wa, twa), ntya = parts_along(Ha, tha);
    std::vector<RegionArg> v;
    v.push_back({ 0, 0, Wa, Ha });
    v.push_back({ 0, 0, 1, 1 });
    v.push_back({ Wa - 1, Ha - 1, 1, 1 });
    {
        const uint32_t w = std::min(twa, Wa), h = std::min(tha, Ha);
        v.push_back({ 1, 1, w > 2 ? w - 2 : 1, h > 2 ? h - 2 : 1 });
    }
    {
        uint32_t x0 = std::min(odd_below(twa), odd_below(Wa)),
                 y0 = std::min(odd_below(tha), odd_below(Ha));
        if (x0 >= Wa)
            x0 = 0;
        if (y0 >= Ha)
            y0 = 0;
        uint32_t w = 5, h = 7;
        while (w > 1 && uint64_t(x0) + w > Wa)
            w -= 2;
        while (h > 1 && uint64_t(y0) + h > Ha)
            h -= 2;
        v.push_back({ x0, y0, w, h });
    }
    v.push_back({ 0, Ha / 2, Wa, 1 });
    v.push_back({ Wa / 2, 0, 1, Ha });
    v.push_back({ (ntxa - 1) * twa, (ntya - 1) * tha, Wa - (ntxa - 1) * twa,
                  Ha - (ntya - 1) * tha });
    if (g.th > unsplit::kSlabRows) {
        auto rows = [&](uint32_t sy0, uint32_t sh) {
            if (uint64_t(sy0) + sh > g.H)
                return;
            const uint32_t other = g.xy ? Ha : Wa;
            const uint32_t o0 = other > 3 ? 3 : 0, on = std::min<uint32_t>(other - o0, 9);
            if (g.xy)
                v.push_back({ sy0, o0, sh, on });
            else
                v.push_back({ o0, sy0, on, sh });
        };
        rows(60, 11);
        if (g.H > g.th + 70)
            rows(g.th + 60, 11);
        const uint32_t cut0 = (g.th - 1) / unsplit::kSlabRows * unsplit::kSlabRows;
        rows(cut0 + 1, std::min(g.th, g.H) - cut0 - 1);
        rows(g.H - 3, 3);
    }
    return v;
}

int
fail(const char* name, uint32_t bpp, const RegionArg& a, const char* what)
{
    std::printf("FAIL %s bpp %u region (%u, %u, %u, %u): %s\n", name, bpp, a.x0, a.y0, a.width,
                a.height, what);
    return 1;
}

int
run_hull(const Case& c, int32_t dtype, int& n_cases)
{
    const ArrayDimensions ad(c.dims, dtype, c.order);
    const uint32_t bpp = uint32_t(bytes_of_type(dtype));
    const unsplit::Geom g = unsplit_geom(ad);
    const uint32_t F = g.n_frames, n = g.n_chunks;
    const uint32_t ranges[3][2] = { { 0, F }, { F / 2, 1 }, { F - 1, 1 } };
    for (const RegionArg& a : regions_of(g)) {
        for (const auto& range : ranges) {
            const uint32_t first = range[0], count = range[1];
            const std::vector<ChunkRange> got = region_chunk_ranges(ad, first, count, &a);
            const std::vector<uint32_t> set = region_chunks(ad, first, count, &a);
            if (got.size() != set.size())
                return fail(c.name, bpp, a, "not the chunks of region_chunks");
            // pixel by pixel, on heap arrays of exactly n entries
            std::unique_ptr<uint64_t[]> lo(new uint64_t[n]), hi(new uint64_t[n]);
            for (uint32_t k = 0; k < n; ++k) {
                lo[k] = ~uint64_t(0);
                hi[k] = 0;
            }
            for (uint32_t f = first; f < first + count; ++f) {
                const uint64_t sf = ad.transpose_frame_id(f);
                const uint32_t grp = ad.tile_group_offset(sf);
                const uint64_t off = ad.chunk_internal_offset(sf);
                for (uint32_t j = 0; j < a.height; ++j)
                    for (uint32_t i = 0; i < a.width; ++i) {
                        const uint32_t ya = a.y0 + j, xa = a.x0 + i; // acquisition
                        const uint32_t sy = g.xy ? xa : ya, sx = g.xy ? ya : xa;
                        const uint32_t chunk = grp + (sy / g.th) * g.ntx + sx / g.tw;
                        if (chunk >= n)
                            return fail(c.name, bpp, a, "a pixel outside the layer");
                        const uint64_t at =
                          off + (uint64_t(sy % g.th) * g.tw + sx % g.tw) * bpp;
                        lo[chunk] = std::min(lo[chunk], at);
                        hi[chunk] = std::max(hi[chunk], at + bpp);
                    }
            }
            for (size_t k = 0; k < got.size(); ++k) {
                const ChunkRange& r = got[k];
                if (r.chunk != set[k] || r.chunk >= n)
                    return fail(c.name, bpp, a, "not the chunks of region_chunks");
                if (r.lo != lo[r.chunk] || r.hi != hi[r.chunk])
                    return fail(c.name, bpp, a, "hull differs from the crop's first and last byte");
                if (r.lo >= r.hi || r.hi > g.bpc)
                    return fail(c.name, bpp, a, "hull outside the chunk");
                hi[r.chunk] = 0;
            }
            for (uint32_t k = 0; k < n; ++k)
                if (hi[k] != 0)
                    return fail(c.name, bpp, a, "a chunk of the crop is missing");
        }
        ++n_cases;
    }
    return 0;
}

uint32_t g_seed = 20240611u;

uint32_t
rnd()
{
    g_seed = g_seed * 1664525u + 1013904223u;
    return g_seed >> 8;
}

void
wr32(uint8_t* p, uint32_t v)
{
    p[0] = uint8_t(v), p[1] = uint8_t(v >> 8), p[2] = uint8_t(v >> 16), p[3] = uint8_t(v >> 24);
}

int
check_ranges(const dec::FrameInfo& h, uint64_t lo, uint64_t hi, int& n_ranges)
{
    const dec::BlockRange b = dec::blocks_of_range(h, lo, hi);
    // block by block
    uint32_t jlo = 0, jhi = 0;
    bool any = false;
    for (uint32_t j = 0; j < h.nblocks; ++j) {
        const uint64_t b0 = uint64_t(j) * h.blocksize;
        const uint64_t b1 = std::min<uint64_t>(b0 + h.blocksize, h.nbytes);
        if (lo < hi && b0 < hi && lo < b1) {
            if (!any)
                jlo = j;
            jhi = j + 1;
            any = true;
        }
    }
    ++n_ranges;
    if (!any) {
        if (b.jlo != b.jhi || b.lo != b.hi) {
            std::printf("FAIL blocks_of_range: blocks for a range that meets none\n");
            return 1;
        }
        return 0;
    }
    const uint64_t s0 = uint64_t(jlo) * h.blocksize;
    const uint64_t s1 = std::min<uint64_t>(uint64_t(jhi) * h.blocksize, h.nbytes);
    if (b.jlo != jlo || b.jhi != jhi || b.lo != s0 || b.hi != s1 || b.lo > lo ||
        b.hi < std::min<uint64_t>(hi, h.nbytes)) {
        std::printf("FAIL blocks_of_range: nbytes %u blocksize %u range [%llu, %llu): blocks "
                    "[%u, %u) span [%llu, %llu), want [%u, %u) [%llu, %llu)\n",
                    h.nbytes, h.blocksize, (unsigned long long)lo, (unsigned long long)hi, b.jlo,
                    b.jhi, (unsigned long long)b.lo, (unsigned long long)b.hi, jlo, jhi,
                    (unsigned long long)s0, (unsigned long long)s1);
        return 1;
    }
    return 0;
}

int
run_headers(int& n_headers, int& n_ranges)
{
    bool saw_big = false, saw_left = false, saw_exact = false;
    for (int it = 0; it < 4000; ++it) {
        const uint32_t ts = 1u << (rnd() % 4);
        uint32_t nbytes, blocksize;
        switch (it % 5) {
            case 0: // a block above the chunk: one leftover block
                nbytes = ts * (1 + rnd() % 300);
                blocksize = nbytes + ts * (1 + rnd() % 7);
                break;
            case 1: // whole blocks only
                blocksize = ts * (1 + rnd() % 64);
                nbytes = blocksize * (1 + rnd() % 40);
                break;
            case 2: // near 2^31: sums past 32 bits
                blocksize = ts * (1u << 20);
                nbytes = 0x7fffffefu - rnd() % 4096;
                break;
            default: // a leftover block
                blocksize = ts * (1 + rnd() % 64);
                nbytes = blocksize * (rnd() % 40) + 1 + rnd() % blocksize;
                break;
        }
        const uint64_t nblocks = (uint64_t(nbytes) + blocksize - 1) / blocksize;
        const uint64_t cbytes = 16 + 4 * nblocks + 8;
        // exactly the header and the block table: parse_header reads no more
        std::unique_ptr<uint8_t[]> f(new uint8_t[16 + 4 * nblocks]);
        f[0] = 2, f[1] = 1, f[2] = uint8_t((dec::kCodecLz4 << 5) | 1u), f[3] = uint8_t(ts);
        wr32(f.get() + 4, nbytes);
        wr32(f.get() + 8, blocksize);
        wr32(f.get() + 12, uint32_t(cbytes));
        for (uint64_t j = 0; j < nblocks; ++j)
            wr32(f.get() + 16 + 4 * j, uint32_t(16 + 4 * nblocks));
        dec::FrameInfo h;
        if (dec::parse_header(f.get(), cbytes, nbytes, h) != dec::kOk || h.nblocks != nblocks) {
            std::printf("FAIL parse_header refused a good header\n");
            return 1;
        }
        saw_big |= blocksize > nbytes;
        saw_left |= h.left != 0 && h.nfull != 0;
        saw_exact |= h.left == 0;
        ++n_headers;
        const uint64_t bs = blocksize, nb = nbytes;
        const uint64_t mid = rnd() % nb;
        const uint64_t edge = nb > bs ? (1 + rnd() % (nb / bs)) * bs : nb; // a block edge
        const uint64_t cases[][2] = {
            { 0, 1 },                 // the first byte
            { nb - 1, nb },           // the last byte, hi == nbytes
            { 0, nb },                // the whole chunk
            { mid, nb },              // hi == nbytes
            { mid, mid },             // empty
            { nb, nb },               // empty, at the end
            { 0, 0 },                 // empty, at the start
            { mid + 1, mid },         // reversed
            { edge - 1, std::min(edge + 1, nb) }, // over a block edge
            { edge, std::min(edge + 1, nb) },     // from a block edge
            { mid, std::min(mid + 1 + rnd() % (2 * bs), nb) },
            { h.nfull * bs, nb },     // the leftover block (empty where there is none)
            { nb, nb + bs },          // past the chunk: no block
            { nb - 1, nb + 3 * bs },  // beyond it: clipped to the last block
        };
        for (const auto& r : cases) {
            if (check_ranges(h, r[0], r[1], n_ranges))
                return 1;
            const uint32_t st = dec::range_status(dec::ByteRange{ r[0], r[1] }, nb);
            const uint32_t want = r[0] > r[1] || r[1] > nb ? dec::kBadHeader
                                  : r[0] == r[1]           ? dec::kNotLoaded
                                                           : dec::kOk;
            if (st != want) {
                std::printf("FAIL range_status\n");
                return 1;
            }
        }
    }
    if (!saw_big || !saw_left || !saw_exact) {
        std::printf("FAIL the headers miss a kind\n");
        return 1;
    }
    // what parse_header leaves of a memcpyed frame has no block
    dec::FrameInfo m{};
    m.nbytes = 100;
    m.blocksize = 10;
    const dec::BlockRange none = dec::blocks_of_range(m, 0, 100);
    if (none.jlo != none.jhi || none.lo != none.hi) {
        std::printf("FAIL blocks of a frame without blocks\n");
        return 1;
    }
    return 0;
}

} // namespace

int
main()
{
    const std::vector<Case> cases = {
        { "aligned", { { kTime, 0, 2, 1 }, { kSpace, 64, 32, 1 }, { kSpace, 64, 32, 2 } }, {} },
        { "ragged", { { kTime, 0, 3, 1 }, { kSpace, 45, 16, 2 }, { kSpace, 70, 32, 1 } }, {} },
        { "odd", { { kTime, 0, 2, 1 }, { kSpace, 17, 17, 1 }, { kSpace, 33, 33, 1 } }, {} },
        { "5d",
          { { kTime, 0, 2, 1 },
            { kChannel, 3, 2, 1 },
            { kSpace, 5, 2, 2 },
            { kSpace, 20, 8, 1 },
            { kSpace, 24, 16, 1 } },
          {} },
        { "5d-permuted",
          { { kTime, 0, 2, 1 },
            { kChannel, 3, 2, 1 },
            { kSpace, 5, 2, 2 },
            { kSpace, 20, 8, 1 },
            { kSpace, 24, 16, 1 } },
          { 0, 2, 1, 3, 4 } },
        { "append-1",
          { { kTime, 0, 1, 1 }, { kSpace, 3, 2, 1 }, { kSpace, 20, 8, 1 }, { kSpace, 24, 16, 1 } },
          {} },
        { "2d", { { kSpace, 45, 16, 1 }, { kSpace, 70, 32, 1 } }, {} },
        { "tall-tiles", { { kTime, 0, 1, 1 }, { kSpace, 150, 100, 1 }, { kSpace, 40, 24, 1 } }, {} },
        { "taller-tiles", { { kTime, 0, 1, 1 }, { kSpace, 250, 100, 1 }, { kSpace, 40, 24, 1 } }, {} },
        { "xy-square",
          { { kTime, 0, 2, 1 }, { kSpace, 64, 32, 1 }, { kSpace, 64, 32, 1 } },
          { 0, 2, 1 } },
        { "xy-ragged",
          { { kTime, 0, 2, 1 }, { kSpace, 45, 16, 1 }, { kSpace, 70, 32, 1 } },
          { 0, 2, 1 } },
        { "xy-tall",
          { { kTime, 0, 1, 1 }, { kSpace, 40, 24, 1 }, { kSpace, 150, 100, 1 } },
          { 0, 2, 1 } },
    };
    const int32_t dtypes[] = { 0, 1, 2, 3 }; // u8, u16, u32, u64
    int n = 0, n_headers = 0, n_ranges = 0;
    try {
        for (const Case& c : cases)
            for (int32_t dt : dtypes)
                if (run_hull(c, dt, n))
                    return 1;
        if (run_headers(n_headers, n_ranges))
            return 1;
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
    std::printf("clean: %d hull cases, %d headers, %d ranges\n", n, n_headers, n_ranges);
    return 0;
}
