// aqz_region.hh -- a region of interest of a chunk layer on the host: the
// un-split geometry of an array and the chunk set of a region, from the tile
// ranges of the map in aqz_unsplit.hh.  No GPU, no HIP: the device reader
// (aqz_reader.cpp), aqz_dims_region_chunks and the host sanitizer program
// (tests/sanitize/region_sanitize.cpp) share this text.
#pragma once

#include "aqz_geometry.hh"
#include "aqz_unsplit.hh"

#include <vector>

namespace aqz {

// A region of interest in pixels of the frames a reader hands back
// (acquisition orientation; aqz_region)
struct RegionArg
{
    uint32_t x0, y0, width, height;
};

// the un-split geometry of one level's array
unsplit::Geom unsplit_geom(const ArrayDimensions& ad);
// The chunks of a layer that hold a pixel of `region` in layer-local frames
// [first, first + count), ascending.  Error(1) for a null or invalid region,
// count == 0 or a range outside frames_per_chunk_layer.
std::vector<uint32_t> region_chunks(const ArrayDimensions& ad, uint32_t first, uint32_t count,
                                    const RegionArg* region);

// A chunk of region_chunks with the byte hull of the window inside it: the
// smallest interval [lo, hi) of chunk bytes that holds every byte a crop of
// `region` from frames [first, first + count) reads (unsplit::region_hull_frame,
// the crop kernel's own map; tab_off need not rise with the frame).
struct ChunkRange
{
    uint32_t chunk;
    uint64_t lo, hi;
};
// The chunks of region_chunks, in its order and with its errors, each with
// its hull; lo < hi <= bytes_per_chunk for every one.
std::vector<ChunkRange> region_chunk_ranges(const ArrayDimensions& ad, uint32_t first,
                                            uint32_t count, const RegionArg* region);

} // namespace aqz
