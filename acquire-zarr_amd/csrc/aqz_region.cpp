// aqz_region.cpp -- see aqz_region.hh.
#include "aqz_region.hh"

namespace aqz {

unsplit::Geom
unsplit_geom(const ArrayDimensions& ad)
{
    unsplit::Geom g{};
    g.W = ad.width_dim().array_size_px;
    g.H = ad.height_dim().array_size_px;
    g.tw = ad.width_dim().chunk_size_px;
    g.th = ad.height_dim().chunk_size_px;
    g.ntx = g.tw ? parts_along(g.W, g.tw) : 0;
    g.nty = g.th ? parts_along(g.H, g.th) : 0;
    g.bpp = uint32_t(bytes_of_type(ad.dtype()));
    g.n_chunks = ad.number_of_chunks_in_memory();
    const uint64_t F = ad.frames_per_chunk_layer();
    g.n_frames = uint32_t(F > 0x7fffffffull ? 0 : F);
    g.xy = ad.needs_xy_transposition() ? 1 : 0;
    g.bpc = ad.bytes_per_chunk();
    return g;
}

std::vector<uint32_t>
region_chunks(const ArrayDimensions& ad, uint32_t first, uint32_t count, const RegionArg* region)
{
    if (!region)
        throw Error(1, "null region");
    const unsplit::Geom g = unsplit_geom(ad);
    if (count == 0 || uint64_t(first) + count > g.n_frames)
        throw Error(1, "frame range empty or outside frames_per_chunk_layer");
    unsplit::Region R;
    if (!unsplit::make_region(g, region->x0, region->y0, region->width, region->height,
                              ~uint64_t(0), R))
        throw Error(1, "region empty or outside the frame");
    std::vector<uint8_t> mark(g.n_chunks, 0);
    for (uint32_t f = first; f < first + count; ++f)
        if (!unsplit::region_mark_chunks(g, R, ad.tile_group_offset(ad.transpose_frame_id(f)),
                                         mark.data()))
            throw Error(9, "the frame tables leave the layer");
    std::vector<uint32_t> out;
    for (uint32_t c = 0; c < g.n_chunks; ++c)
        if (mark[c])
            out.push_back(c);
    return out;
}

std::vector<ChunkRange>
region_chunk_ranges(const ArrayDimensions& ad, uint32_t first, uint32_t count,
                    const RegionArg* region)
{
    if (!region)
        throw Error(1, "null region");
    const unsplit::Geom g = unsplit_geom(ad);
    if (count == 0 || uint64_t(first) + count > g.n_frames)
        throw Error(1, "frame range empty or outside frames_per_chunk_layer");
    unsplit::Region R;
    if (!unsplit::make_region(g, region->x0, region->y0, region->width, region->height,
                              ~uint64_t(0), R))
        throw Error(1, "region empty or outside the frame");
    // region_rect bounds the destination too: a crop with rows back to back
    unsplit::make_region(g, region->x0, region->y0, region->width, region->height,
                         uint64_t(unsplit::region_width(g, R)) * g.bpp, R);
    std::vector<uint64_t> lo(g.n_chunks, ~uint64_t(0)), hi(g.n_chunks, 0);
    for (uint32_t f = first; f < first + count; ++f) {
        const uint64_t s = ad.transpose_frame_id(f);
        if (!unsplit::region_hull_frame(g, R, ad.tile_group_offset(s), ad.chunk_internal_offset(s),
                                        lo.data(), hi.data()))
            throw Error(9, "the frame tables leave the layer");
    }
    std::vector<ChunkRange> out;
    for (uint32_t c = 0; c < g.n_chunks; ++c)
        if (lo[c] < hi[c])
            out.push_back(ChunkRange{ c, lo[c], hi[c] });
    return out;
}

} // namespace aqz
