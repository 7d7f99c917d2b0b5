// unsplit_sanitize.cpp -- the device reader's address map (csrc/aqz_unsplit.hh:
// tile rectangles, slabs, the XY swap, every source and destination bound) run
// on the host under ASan + UBSan with a serial byte mover.
//
// For each geometry, seeded frames of two chunk layers are split into chunks
// by the product's host split (aqz::split_rows; for the XY-swapped storage
// order the frame is first transposed as transpose_frame, array.cpp:488-534,
// does, since the host split refuses XY).  Every chunk is then copied into a
// heap buffer of exactly bytes_per_chunk and un-split into heap frames of
// exactly W * H * bpp bytes, so that any read or write past an end is a
// sanitizer report.  The frames must equal the input; a chunk left out reads
// as zeros.
#include "aqz_geometry.hh"
#include "aqz_hostsplit.hh"
#include "aqz_unsplit.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace aqz;

namespace {

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
fail(const char* name, uint32_t bpp, const char* what)
{
    std::printf("FAIL %s bpp %u: %s\n", name, bpp, what);
    return 1;
}

int
run(const Case& c, int32_t dtype)
{
    const ArrayDimensions ad(c.dims, dtype, c.order);
    const uint32_t bpp = uint32_t(bytes_of_type(dtype));
    unsplit::Geom g{};
    g.W = ad.width_dim().array_size_px;
    g.H = ad.height_dim().array_size_px;
    g.tw = ad.width_dim().chunk_size_px;
    g.th = ad.height_dim().chunk_size_px;
    g.ntx = parts_along(g.W, g.tw);
    g.nty = parts_along(g.H, g.th);
    g.bpp = bpp;
    g.n_chunks = ad.number_of_chunks_in_memory();
    g.n_frames = uint32_t(ad.frames_per_chunk_layer());
    g.xy = ad.needs_xy_transposition() ? 1 : 0;
    g.bpc = ad.bytes_per_chunk();
    const uint64_t fb = unsplit::frame_bytes(g);
    const uint32_t F = g.n_frames, n = g.n_chunks;

    // the split side: for XY an array of the storage dims (no frame permutation
    // goes with the cases' XY orders) fed transposed frames
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

    uint32_t seed = 12345u + bpp;
    for (uint32_t layer = 0; layer < 2; ++layer) {
        std::vector<std::unique_ptr<uint8_t[]>> frames(F);
        std::vector<uint8_t> packed(size_t(n) * g.bpc, 0), has(n, 0), xframe(fb);
        for (uint32_t f = 0; f < F; ++f) {
            frames[f].reset(new uint8_t[fb]);
            for (uint64_t i = 0; i < fb; ++i) {
                seed = seed * 1664525u + 1013904223u;
                frames[f][i] = uint8_t((seed >> 24) | 1u); // never zero: has_data is set
            }
            const uint8_t* in = frames[f].get();
            if (g.xy) {
                // acquisition H_a = W rows of W_a = H pixels -> storage H rows of W
                for (uint32_t y = 0; y < g.W; ++y)
                    for (uint32_t x = 0; x < g.H; ++x)
                        std::memcpy(&xframe[(uint64_t(x) * g.W + y) * bpp],
                                    in + (uint64_t(y) * g.H + x) * bpp, bpp);
                in = xframe.data();
            }
            const SplitGeom sg = split_geom(sad, uint64_t(layer) * F + f);
            split_rows(sg, in, 0, g.H, packed.data(), 0, n, has.data());
        }
        // chunk n - 1 of layer 1 is left out: it reads as zeros
        const uint32_t dropped = layer == 1 ? n - 1 : n;
        std::vector<std::unique_ptr<uint8_t[]>> chunks(n);
        std::vector<uint64_t> chunk_src(n, unsplit::kNoChunk);
        for (uint32_t k = 0; k < n; ++k) {
            if (!has[k])
                return fail(c.name, bpp, "a chunk got no data");
            if (k == dropped)
                continue;
            chunks[k].reset(new uint8_t[g.bpc]);
            std::memcpy(chunks[k].get(), &packed[size_t(k) * g.bpc], g.bpc);
            chunk_src[k] = uint64_t(reinterpret_cast<uintptr_t>(chunks[k].get()));
        }
        for (uint32_t f = 0; f < F; ++f) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[fb]);
            std::memset(out.get(), 0xA5, fb);
            HostMover m{ out.get(), bpp };
            uint64_t moved = 0;
            for (uint64_t it = 0; it < unsplit::items_per_frame(g); ++it) {
                const uint32_t st =
                  g.xy ? unsplit::unsplit_item<true>(g, tab_grp.data(), tab_off.data(),
                                                     chunk_src.data(), f, it, m)
                       : unsplit::unsplit_item<false>(g, tab_grp.data(), tab_off.data(),
                                                      chunk_src.data(), f, it, m);
                if (st == unsplit::kBad)
                    return fail(c.name, bpp, "the map refused an item of a consistent geometry");
                moved += st == unsplit::kMove;
            }
            if (moved == 0)
                return fail(c.name, bpp, "nothing moved");
            if (dropped == n) {
                if (std::memcmp(out.get(), frames[f].get(), fb) != 0)
                    return fail(c.name, bpp, "frame differs from the input");
                continue;
            }
            // pixels of the dropped chunk are zero, every other pixel exact
            const uint64_t sf = ad.transpose_frame_id(f);
            const uint32_t grp = ad.tile_group_offset(sf);
            for (uint32_t y = 0; y < g.H; ++y)
                for (uint32_t x = 0; x < g.W; ++x) {
                    const uint32_t k = grp + (y / g.th) * g.ntx + x / g.tw;
                    const uint64_t at =
                      g.xy ? (uint64_t(x) * g.H + y) * bpp : (uint64_t(y) * g.W + x) * bpp;
                    for (uint32_t b = 0; b < bpp; ++b) {
                        const uint8_t want = k == dropped ? 0 : frames[f][at + b];
                        if (out[at + b] != want)
                            return fail(c.name, bpp, "pixel differs with a chunk left out");
                    }
                }
        }
    }
    // what the map must refuse: items and frames outside the layer, a chunk
    // table shorter than the geometry says
    HostMover none{ nullptr, bpp };
    std::vector<uint64_t> no_src(n, unsplit::kNoChunk);
    unsplit::Geom small = g;
    small.n_chunks = 0;
    unsplit::Geom shortc = g;
    shortc.bpc = g.bpc - 1;
    bool refused = true;
    if (g.xy) {
        refused &= unsplit::unsplit_item<true>(g, tab_grp.data(), tab_off.data(), no_src.data(), F,
                                               0, none) == unsplit::kBad;
        refused &= unsplit::unsplit_item<true>(g, tab_grp.data(), tab_off.data(), no_src.data(), 0,
                                               unsplit::items_per_frame(g), none) == unsplit::kBad;
        refused &= unsplit::unsplit_item<true>(small, tab_grp.data(), tab_off.data(),
                                               no_src.data(), 0, 0, none) == unsplit::kBad;
    } else {
        refused &= unsplit::unsplit_item<false>(g, tab_grp.data(), tab_off.data(), no_src.data(),
                                                F, 0, none) == unsplit::kBad;
        refused &= unsplit::unsplit_item<false>(g, tab_grp.data(), tab_off.data(), no_src.data(),
                                                0, unsplit::items_per_frame(g),
                                                none) == unsplit::kBad;
        refused &= unsplit::unsplit_item<false>(small, tab_grp.data(), tab_off.data(),
                                                no_src.data(), 0, 0, none) == unsplit::kBad;
        refused &= unsplit::unsplit_item<true>(g, tab_grp.data(), tab_off.data(), no_src.data(), 0,
                                               0, none) == unsplit::kBad;
    }
    // the last tile row of the last frame ends at the chunk's last byte
    unsplit::Rect r;
    bool hit_end = false;
    for (uint32_t f = 0; f < F; ++f)
        for (uint32_t s = 0; s < unsplit::slabs_per_tile(g); ++s)
            if (unsplit::tile_rect(shortc, tab_grp[f], tab_off[f], 0, 0, s, r) == unsplit::kBad)
                hit_end = true;
    if (g.H >= g.th && g.W >= g.tw && !hit_end)
        return fail(c.name, bpp, "a chunk one byte short was not refused");
    if (!refused)
        return fail(c.name, bpp, "an item outside the layer was not refused");
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
    for (const Case& c : cases)
        for (int32_t dt : dtypes) {
            if (run(c, dt))
                return 1;
            ++n;
        }
    std::printf("clean: %d cases\n", n);
    return 0;
}
