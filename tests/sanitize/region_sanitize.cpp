// region_sanitize.cpp -- the region part of the device reader's address map
// (csrc/aqz_unsplit.hh: make_region, the item walk of a region, region_rect)
// and the chunk set of a region (csrc/aqz_region.cpp) run on the host under
// ASan + UBSan with a serial byte mover.
//
// For each geometry of unsplit_sanitize.cpp, one taller, and each element size, seeded
// frames of one chunk layer are split into chunks by the product's host split
// (aqz::split_rows; XY frames transposed first, as there).  Then, per region,
// frame range and destination shape: every chunk of region_chunks becomes a
// heap block of exactly bytes_per_chunk, every other chunk is NOT allocated
// at all (its chunk_src entry is an address nothing may touch), and the
// destination is a heap block of exactly (count - 1) * frame_stride +
// (height - 1) * row_stride + width * bpp bytes painted with a fill, so that
// any access outside the window or the crop is a sanitizer report.  The
// output must equal the crop; every byte between rows and frames keeps the
// fill.
#include "aqz_geometry.hh"
#include "aqz_hostsplit.hh"
#include "aqz_region.hh"
#include "aqz_unsplit.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <vector>

using namespace aqz;

namespace {

constexpr uint8_t kFill = 0xA5;

struct HostMover
{
    uint8_t* dst;
    uint32_t bpp;
    // chunk_src holds addresses: every chunk is a heap block of its own
    static const uint8_t* at(uint64_t a) { return reinterpret_cast<const uint8_t*>(uintptr_t(a)); }
    void copy(uint64_t base, const unsplit::Rect& r)
    {
        for (uint32_t y = 0; y < r.rows; ++y)
            std::memcpy(dst + r.dst + y * r.dst_pitch, at(base + r.src + y * r.src_pitch),
                        r.dst_row_bytes);
    }
    void transpose(uint64_t base, const unsplit::Rect& r)
    {
        for (uint32_t y = 0; y < r.rows; ++y)
            for (uint32_t x = 0; x < r.cols; ++x)
                std::memcpy(dst + r.dst + x * r.dst_pitch + uint64_t(y) * bpp,
                            at(base + r.src + y * r.src_pitch + uint64_t(x) * bpp), bpp);
    }
    void zero(const unsplit::Rect& r)
    {
        for (uint32_t y = 0; y < r.dst_rows; ++y)
            std::memset(dst + r.dst + y * r.dst_pitch, 0, r.dst_row_bytes);
    }
};

struct Case
{
    const char* name;
    std::vector<Dim> dims;
    std::vector<size_t> order;
};

int
fail(const char* name, uint32_t bpp, const RegionArg& a, const char* what)
{
    std::printf("FAIL %s bpp %u region (%u, %u, %u, %u): %s\n", name, bpp, a.x0, a.y0, a.width,
                a.height, what);
    return 1;
}

uint32_t
odd_below(uint32_t v) // the largest odd number below v, 1 at the least
{
    if (v < 3)
        return 1;
    return (v - 1) % 2 ? v - 1 : v - 2;
}

// The regions of one geometry, in pixels of the frames handed back: Wa x Ha
// pixels in tiles of twa x tha; storage tiles taller than a slab add the
// slab cases.
std::vector<RegionArg>
regions_of(const unsplit::Geom& g)
{
    const uint32_t Wa = g.xy ? g.H : g.W, Ha = g.xy ? g.W : g.H;
    const uint32_t twa = g.xy ? g.th : g.tw, tha = g.xy ? g.tw : g.th;
    const uint32_t ntxa = parts_along(Wa, twa), ntya = parts_along(Ha, tha);
    std::vector<RegionArg> v;
    v.push_back({ 0, 0, Wa, Ha });          // the whole frame
    v.push_back({ 0, 0, 1, 1 });            // one pixel, first
    v.push_back({ Wa - 1, Ha - 1, 1, 1 });  // one pixel, last
    {
        // strictly inside tile (0, 0)
        const uint32_t w = std::min(twa, Wa), h = std::min(tha, Ha);
        v.push_back({ 1, 1, w > 2 ? w - 2 : 1, h > 2 ? h - 2 : 1 });
    }
    {
        // over the four-tile corner at (twa, tha) where the frame has one:
        // odd origin, odd width and height
        uint32_t x0 = std::min(odd_below(twa), odd_below(Wa)), y0 = std::min(odd_below(tha), odd_below(Ha));
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
    v.push_back({ 0, Ha / 2, Wa, 1 }); // one full-width row
    v.push_back({ Wa / 2, 0, 1, Ha }); // one full-height column
    // the last tile in x and in y, ragged where the geometry is
    v.push_back({ (ntxa - 1) * twa, (ntya - 1) * tha, Wa - (ntxa - 1) * twa,
                  Ha - (ntya - 1) * tha });
    if (g.th > unsplit::kSlabRows) {
        // storage rows 60-70 of the last tile row that has them (they cross a
        // slab boundary), and the rows of a tile's cut last slab
        auto rows = [&](uint32_t sy0, uint32_t sh) {
            if (uint64_t(sy0) + sh > g.H)
                return;
            const uint32_t other = g.xy ? Ha : Wa; // the axis the rows do not run along
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
        rows(g.H - 3, 3); // the frame's last rows: the last tile row's last slab
    }
    return v;
}

int
run(const Case& c, int32_t dtype, int& n_cases)
{
    const ArrayDimensions ad(c.dims, dtype, c.order);
    const uint32_t bpp = uint32_t(bytes_of_type(dtype));
    const unsplit::Geom g = unsplit_geom(ad);
    const uint64_t fb = unsplit::frame_bytes(g);
    const uint32_t F = g.n_frames, n = g.n_chunks;
    const uint32_t Wa = g.xy ? g.H : g.W; // pixels per row of the frames handed back

    std::unique_ptr<ArrayDimensions> storage;
    if (g.xy)
        storage = std::make_unique<ArrayDimensions>(ad.dims(), dtype);
    const ArrayDimensions& sad = g.xy ? *storage : ad;

    std::vector<uint32_t> tab_grp(F);
    std::vector<uint64_t> tab_off(F);
    for (uint32_t f = 0; f < F; ++f) {
        const uint64_t sf = ad.transpose_frame_id(f);
        tab_grp[f] = ad.tile_group_offset(sf);
        tab_off[f] = ad.chunk_internal_offset(sf);
    }

    // one layer of frames, split
    uint32_t seed = 4321u + bpp;
    std::vector<std::vector<uint8_t>> frames(F, std::vector<uint8_t>(fb));
    std::vector<uint8_t> packed(size_t(n) * g.bpc, 0), has(n, 0), xframe(fb);
    for (uint32_t f = 0; f < F; ++f) {
        for (uint64_t i = 0; i < fb; ++i) {
            seed = seed * 1664525u + 1013904223u;
            frames[f][i] = uint8_t((seed >> 24) | 1u);
        }
        const uint8_t* in = frames[f].data();
        if (g.xy) {
            for (uint32_t y = 0; y < g.W; ++y)
                for (uint32_t x = 0; x < g.H; ++x)
                    std::memcpy(&xframe[(uint64_t(x) * g.W + y) * bpp],
                                in + (uint64_t(y) * g.H + x) * bpp, bpp);
            in = xframe.data();
        }
        split_rows(split_geom(sad, f), in, 0, g.H, packed.data(), 0, n, has.data());
    }

    const uint32_t ranges[3][2] = { { 0, F }, { F / 2, 1 }, { F - 1, 1 } };
    for (const RegionArg& a : regions_of(g)) {
        for (const auto& range : ranges) {
            const uint32_t first = range[0], count = range[1];
            const std::vector<uint32_t> set = region_chunks(ad, first, count, &a);
            if (set.empty())
                return fail(c.name, bpp, a, "empty chunk set");
            for (size_t i = 1; i < set.size(); ++i)
                if (set[i] <= set[i - 1])
                    return fail(c.name, bpp, a, "chunk set not ascending");
            // only the chunks of the set exist; the others must never be addressed
            std::vector<std::unique_ptr<uint8_t[]>> chunks(n);
            std::vector<uint64_t> chunk_src(n, uint64_t(16)); // an address nothing may touch
            for (uint32_t k : set) {
                if (k >= n)
                    return fail(c.name, bpp, a, "chunk outside the layer");
                chunks[k].reset(new uint8_t[g.bpc]);
                std::memcpy(chunks[k].get(), &packed[size_t(k) * g.bpc], g.bpc);
                chunk_src[k] = uint64_t(reinterpret_cast<uintptr_t>(chunks[k].get()));
            }
            // the last chunk of the set reads as zeros in a second pass
            for (int dropped = 0; dropped < 2; ++dropped) {
                const uint32_t drop = dropped ? set.back() : n;
                if (dropped)
                    chunk_src[drop] = unsplit::kNoChunk;
                for (int padded = 0; padded < 2; ++padded) {
                    const uint64_t row_bytes = uint64_t(a.width) * bpp;
                    const uint64_t row_stride = row_bytes + (padded ? 5 : 0);
                    const uint64_t extent = (uint64_t(a.height) - 1) * row_stride + row_bytes;
                    const uint64_t frame_stride = extent + (padded ? 7 : 0);
                    const uint64_t total = (uint64_t(count) - 1) * frame_stride + extent;
                    std::unique_ptr<uint8_t[]> out(new uint8_t[total]);
                    std::memset(out.get(), kFill, total);
                    unsplit::Region R;
                    if (!unsplit::make_region(g, a.x0, a.y0, a.width, a.height, row_stride, R))
                        return fail(c.name, bpp, a, "a valid region was refused");
                    if (unsplit::region_frame_extent(g, R) != extent)
                        return fail(c.name, bpp, a, "frame extent");
                    const uint64_t items = unsplit::region_items_per_frame(g, R);
                    if (items == 0 || items > unsplit::items_per_frame(g))
                        return fail(c.name, bpp, a, "item count");
                    for (uint32_t k = 0; k < count; ++k) {
                        HostMover m{ out.get() + k * frame_stride, bpp };
                        uint64_t moved = 0;
                        for (uint64_t it = 0; it < items; ++it) {
                            const uint32_t st =
                              g.xy ? unsplit::region_item<true>(g, R, tab_grp.data(),
                                                                tab_off.data(), chunk_src.data(),
                                                                first + k, it, m)
                                   : unsplit::region_item<false>(g, R, tab_grp.data(),
                                                                 tab_off.data(),
                                                                 chunk_src.data(), first + k,
                                                                 it, m);
                            if (st == unsplit::kBad)
                                return fail(c.name, bpp, a, "the map refused an item");
                            moved += st == unsplit::kMove;
                        }
                        if (moved == 0)
                            return fail(c.name, bpp, a, "nothing moved");
                        // items outside the walk are refused
                        if ((g.xy ? unsplit::region_item<true>(g, R, tab_grp.data(),
                                                               tab_off.data(), chunk_src.data(),
                                                               first + k, items, m)
                                  : unsplit::region_item<false>(g, R, tab_grp.data(),
                                                                tab_off.data(), chunk_src.data(),
                                                                first + k, items, m)) !=
                            unsplit::kBad)
                            return fail(c.name, bpp, a, "an item outside the walk was taken");
                    }
                    // the crop, pixel by pixel; the fill everywhere else
                    std::vector<uint8_t> want(total, kFill);
                    for (uint32_t k = 0; k < count; ++k) {
                        const uint32_t f = first + k;
                        const uint32_t grp = tab_grp[f];
                        for (uint32_t j = 0; j < a.height; ++j)
                            for (uint32_t i = 0; i < a.width; ++i) {
                                const uint32_t ya = a.y0 + j, xa = a.x0 + i; // acquisition
                                const uint32_t sy = g.xy ? xa : ya, sx = g.xy ? ya : xa;
                                const uint32_t chunk = grp + (sy / g.th) * g.ntx + sx / g.tw;
                                const uint8_t* px =
                                  &frames[f][(uint64_t(ya) * Wa + xa) * bpp];
                                uint8_t* w =
                                  &want[k * frame_stride + j * row_stride + uint64_t(i) * bpp];
                                for (uint32_t b = 0; b < bpp; ++b)
                                    w[b] = chunk == drop ? 0 : px[b];
                            }
                    }
                    if (std::memcmp(out.get(), want.data(), total) != 0)
                        return fail(c.name, bpp, a,
                                    dropped ? "crop differs with a chunk left out"
                                            : "crop or fill differs");
                }
            }
        }
        // what the map refuses: a row pitch below the row, regions that leave
        // the frame (the sums in 64 bits), empty regions
        unsplit::Region R;
        const RegionArg bad[] = { { a.x0, a.y0, 0, a.height },
                                  { a.x0, a.y0, a.width, 0 },
                                  { 0xffffffffu, a.y0, 2, a.height },
                                  { a.x0, 0xffffffffu, a.width, 2 },
                                  { a.x0, a.y0, Wa - a.x0 + 1, a.height } };
        for (const RegionArg& b : bad)
            if (unsplit::make_region(g, b.x0, b.y0, b.width, b.height, ~uint64_t(0), R))
                return fail(c.name, bpp, b, "an invalid region was accepted");
        if (unsplit::make_region(g, a.x0, a.y0, a.width, a.height, uint64_t(a.width) * bpp - 1,
                                 R))
            return fail(c.name, bpp, a, "a row pitch below the row was accepted");
        ++n_cases;
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
        // beyond unsplit_sanitize.cpp's list: three tile rows of two slabs, so that rows
        // 60-70 of tile row 1 exist and a column walks a whole interior tile row
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
    int n = 0;
    try {
        for (const Case& c : cases)
            for (int32_t dt : dtypes)
                if (run(c, dt, n))
                    return 1;
    } catch (const std::exception& e) {
        std::printf("FAIL: %s\n", e.what());
        return 1;
    }
    std::printf("clean: %d cases\n", n);
    return 0;
}
