// aqz_unsplit.hh -- the address map of the device reader's un-split kernel
// (aqz_unsplit.hip), compiled for host and device from this one text: which
// bytes of which chunk are which bytes of a row-major frame, with every bound
// it enforces.  It is the inverse of Array::write_frame_to_chunks_
// (array.cpp:537-619) with Chunk::write_tile_rows (chunk.cpp:17-58) -- the
// tile stores of the fused kernels and of aqz_hostsplit.cpp -- and, for the
// XY-transposed storage order, of transpose_frame (array.cpp:488-534).
// Only the byte movers differ (the Mover argument of unsplit_item): a serial
// loop on the host (tests/sanitize/unsplit_sanitize.cpp runs this text under
// a host sanitizer), the 256 threads of a workgroup on the device.
//
// The map.  Frame f of a layer (layer-local id, acquisition order) has the
// storage id s = transpose_frame_id(f); tab_grp[f] = tile_group_offset(s) and
// tab_off[f] = chunk_internal_offset(s), the tables of the stage.  Tile
// (ty, tx) of the frame lies in chunk tab_grp[f] + ty * ntx + tx; row r of
// the tile starts at tab_off[f] + r * tw * bpp inside the chunk and carries
// min(tw, W - tx * tw) valid pixels; rows >= H - ty * th do not exist, and
// the ragged padding of a chunk is never read.  With the XY-transposed
// storage order, storage pixel (y, x) is acquisition pixel (x, y): the frame
// handed back has W rows of H pixels.
#pragma once

#include <cstdint>

#ifndef AQZ_HD
#if defined(__HIP__) || defined(__CUDACC__)
#define AQZ_HD __host__ __device__
#else
#define AQZ_HD
#endif
#endif

namespace aqz {
namespace unsplit {

// chunk_src entry of a chunk that was never written: its pixels read as
// zeros (fill_value 0, array.cpp:279)
constexpr uint64_t kNoChunk = ~uint64_t(0);

// rows of a tile one work item moves (also the edge of the LDS transpose tile)
constexpr uint32_t kSlabRows = 64;

enum : uint32_t
{
    kEmpty = 0, // the item holds no pixel (rows past the frame's last row)
    kMove = 1,  // the rectangle was handed to the mover
    kBad = 2,   // geometry and tables disagree: nothing was moved
};

struct Geom
{
    uint32_t W, H;     // storage frame: pixels per row, rows
    uint32_t tw, th;   // tile (chunk) pixels per row, rows
    uint32_t ntx, nty; // tiles per frame
    uint32_t bpp;      // bytes per pixel
    uint32_t n_chunks; // chunks per layer
    uint32_t n_frames; // frames per layer
    uint32_t xy;       // 1: the storage order swaps y and x
    uint64_t bpc;      // bytes per chunk
};

AQZ_HD inline uint32_t
slabs_per_tile(const Geom& g)
{
    return (g.th + kSlabRows - 1) / kSlabRows;
}

// work items of one frame: (ty, tx, slab) with the slab fastest
AQZ_HD inline uint64_t
items_per_frame(const Geom& g)
{
    return uint64_t(g.ntx) * g.nty * slabs_per_tile(g);
}

AQZ_HD inline uint64_t
frame_bytes(const Geom& g)
{
    return uint64_t(g.W) * g.H * g.bpp;
}

// One rectangle of pixels: `rows` rows of `cols` storage pixels inside a
// chunk, and where they go inside the destination frame.
struct Rect
{
    uint32_t chunk;         // of the layer
    uint32_t rows, cols;    // storage rows (<= kSlabRows) and pixels per row
    uint64_t src;           // first byte, inside the chunk
    uint64_t src_pitch;     // bytes from row to row inside the chunk
    uint64_t dst;           // first byte, inside the destination frame
    uint64_t dst_pitch;     // bytes from destination row to destination row
    uint32_t dst_rows;      // rows (xy: cols) ...
    uint64_t dst_row_bytes; // ... of cols * bpp (xy: rows * bpp) bytes
};

// The rectangle of slab `slab` of tile (ty, tx) of a frame whose tile 0 lies
// in chunk `grp` at byte `internal`.  kMove only when every source byte lies
// inside [0, bpc) of a chunk below n_chunks and every destination byte inside
// [0, W * H * bpp).
AQZ_HD inline uint32_t
tile_rect(const Geom& g, uint32_t grp, uint64_t internal, uint32_t ty, uint32_t tx,
          uint32_t slab, Rect& r)
{
    if (ty >= g.nty || tx >= g.ntx || g.bpp == 0 || g.tw == 0 || g.th == 0)
        return kBad;
    const uint64_t r0 = uint64_t(slab) * kSlabRows; // first row, inside the tile
    const uint64_t y0 = uint64_t(ty) * g.th + r0;   // ... and inside the frame
    const uint64_t x0 = uint64_t(tx) * g.tw;
    if (x0 >= g.W)
        return kBad;
    if (r0 >= g.th || y0 >= g.H)
        return kEmpty;
    uint64_t rows = g.th - r0;
    if (rows > kSlabRows)
        rows = kSlabRows;
    if (rows > g.H - y0)
        rows = g.H - y0;
    uint64_t cols = g.W - x0;
    if (cols > g.tw)
        cols = g.tw;
    const uint64_t chunk = uint64_t(grp) + uint64_t(ty) * g.ntx + tx;
    if (chunk >= g.n_chunks)
        return kBad;
    r.chunk = uint32_t(chunk);
    r.rows = uint32_t(rows);
    r.cols = uint32_t(cols);
    r.src_pitch = uint64_t(g.tw) * g.bpp;
    r.src = internal + r0 * r.src_pitch;
    if (r.src + (rows - 1) * r.src_pitch + cols * g.bpp > g.bpc)
        return kBad;
    if (!g.xy) {
        r.dst_pitch = uint64_t(g.W) * g.bpp;
        r.dst = y0 * r.dst_pitch + x0 * g.bpp;
        r.dst_rows = r.rows;
        r.dst_row_bytes = cols * g.bpp;
    } else {
        // storage pixel (y, x) -> row x, pixel y of a frame of W rows of H
        r.dst_pitch = uint64_t(g.H) * g.bpp;
        r.dst = x0 * r.dst_pitch + y0 * g.bpp;
        r.dst_rows = r.cols;
        r.dst_row_bytes = rows * g.bpp;
    }
    if (r.dst + (uint64_t(r.dst_rows) - 1) * r.dst_pitch + r.dst_row_bytes > frame_bytes(g))
        return kBad;
    return kMove;
}

// Work item `item` (< items_per_frame) of layer-local frame `frame`: its
// rectangle goes to the mover -- copy(base, r) (XY: transpose(base, r)) for a
// chunk at byte `base` of the source, zero(r) for a chunk never written.
// The mover holds the source and the destination frame; the rectangle it
// gets is inside both.
template<bool XY, class Mover>
AQZ_HD inline uint32_t
unsplit_item(const Geom& g, const uint32_t* tab_grp, const uint64_t* tab_off,
             const uint64_t* chunk_src, uint32_t frame, uint64_t item, Mover& m)
{
    if (frame >= g.n_frames || item >= items_per_frame(g) || XY != (g.xy != 0))
        return kBad;
    const uint32_t spt = slabs_per_tile(g);
    const uint32_t slab = uint32_t(item % spt);
    const uint64_t t = item / spt;
    const uint32_t ty = uint32_t(t / g.ntx), tx = uint32_t(t % g.ntx);
    Rect r;
    const uint32_t st = tile_rect(g, tab_grp[frame], tab_off[frame], ty, tx, slab, r);
    if (st != kMove)
        return st;
    const uint64_t base = chunk_src[r.chunk];
    if (base == kNoChunk)
        m.zero(r);
    else if constexpr (XY)
        m.transpose(base, r);
    else
        m.copy(base, r);
    return kMove;
}

// Bytes the copy path may move at a time: the largest power of two up to 16
// that divides every row start and row length on both sides.  `align` is
// the OR of the source address, every chunk_src entry (or the chunk pitch),
// the destination address and the destination stride; chunk-internal
// offsets are multiples of tw * bpp.
inline uint32_t
copy_unit(const Geom& g, uint64_t align)
{
    const uint64_t a = align | uint64_t(g.tw) * g.bpp | uint64_t(g.W) * g.bpp | 16u;
    return uint32_t(a & (~a + 1));
}

// XY path: may pixels be moved as words of bpp bytes?
inline bool
pixel_aligned(const Geom& g, uint64_t align)
{
    return g.bpp != 0 && (align & (g.bpp - 1)) == 0;
}

// One launch: frames [first, first + count) of the layer -> dst + i * dst_stride
struct Params
{
    Geom g;
    const uint8_t* src;        // chunk c at src + chunk_src[c]
    const uint64_t* chunk_src; // [n_chunks] byte offsets, kNoChunk = never written
    const uint32_t* tab_grp;   // [n_frames]
    const uint64_t* tab_off;   // [n_frames]
    uint8_t* dst;
    uint64_t dst_stride;       // >= frame_bytes(g)
    uint32_t first, count;
};

// ---- region reads ---------------------------------------------------------
// A crop of frames: the same map, walked only over the tiles and slabs that
// meet the region, each rectangle clipped to it and the destination rebased
// to the region's origin with the caller's row pitch.
//
// The region in storage coordinates (make_region applies the XY swap once,
// on the host, as Geom::xy is applied), with the ranges the walk needs.
struct Region
{
    uint32_t x0, y0, w, h;     // storage columns [x0, x0 + w), rows [y0, y0 + h)
    uint32_t tx0, ntx;         // tile columns tx0 .. tx0 + ntx - 1 meet it
    uint32_t ty0, nty;         // tile rows ty0 .. ty0 + nty - 1 meet it
    uint32_t s0;               // first slab of tile row ty0 that meets it
    uint32_t n_first, n_last;  // slabs of the first / the last tile row that meet it
    uint64_t row_pitch;        // bytes from destination row to destination row
};

// pixels per row and rows of the crop handed back (acquisition orientation)
AQZ_HD inline uint32_t
region_width(const Geom& g, const Region& R)
{
    return g.xy ? R.h : R.w;
}

AQZ_HD inline uint32_t
region_height(const Geom& g, const Region& R)
{
    return g.xy ? R.w : R.h;
}

// bytes of one destination frame that a read may write: the last row is cut
AQZ_HD inline uint64_t
region_frame_extent(const Geom& g, const Region& R)
{
    return (uint64_t(region_height(g, R)) - 1) * R.row_pitch +
           uint64_t(region_width(g, R)) * g.bpp;
}

AQZ_HD inline bool
region_valid(const Geom& g, const Region& R)
{
    if (R.w == 0 || R.h == 0 || g.tw == 0 || g.th == 0 || g.bpp == 0)
        return false;
    if (uint64_t(R.x0) + R.w > g.W || uint64_t(R.y0) + R.h > g.H)
        return false;
    const uint32_t x1 = R.x0 + R.w - 1, y1 = R.y0 + R.h - 1;
    if (R.tx0 != R.x0 / g.tw || R.ntx != x1 / g.tw - R.tx0 + 1)
        return false;
    if (R.ty0 != R.y0 / g.th || R.nty != y1 / g.th - R.ty0 + 1)
        return false;
    const uint32_t s0 = (R.y0 - R.ty0 * g.th) / kSlabRows;
    const uint32_t s1 = (y1 - (R.ty0 + R.nty - 1) * g.th) / kSlabRows; // of the last tile row
    if (R.s0 != s0 || R.n_last != s1 + 1 - (R.nty == 1 ? s0 : 0))
        return false;
    if (R.n_first != (R.nty == 1 ? R.n_last : slabs_per_tile(g) - s0))
        return false;
    return R.row_pitch >= uint64_t(region_width(g, R)) * g.bpp;
}

// The region (x0, y0, width, height) in pixels of the frames handed back
// (acquisition orientation) -> storage coordinates and walk ranges.  False
// when it is empty or leaves the frame; the sums are taken in 64 bits.
inline bool
make_region(const Geom& g, uint32_t x0, uint32_t y0, uint32_t width, uint32_t height,
            uint64_t row_pitch, Region& R)
{
    R = Region{};
    if (g.xy) {
        R.x0 = y0, R.w = height;
        R.y0 = x0, R.h = width;
    } else {
        R.x0 = x0, R.w = width;
        R.y0 = y0, R.h = height;
    }
    if (R.w == 0 || R.h == 0 || g.tw == 0 || g.th == 0 || g.bpp == 0)
        return false;
    if (uint64_t(R.x0) + R.w > g.W || uint64_t(R.y0) + R.h > g.H)
        return false;
    const uint32_t x1 = R.x0 + R.w - 1, y1 = R.y0 + R.h - 1;
    R.tx0 = R.x0 / g.tw;
    R.ntx = x1 / g.tw - R.tx0 + 1;
    R.ty0 = R.y0 / g.th;
    R.nty = y1 / g.th - R.ty0 + 1;
    R.s0 = (R.y0 - R.ty0 * g.th) / kSlabRows;
    const uint32_t s1 = (y1 - (R.ty0 + R.nty - 1) * g.th) / kSlabRows;
    R.n_last = s1 + 1 - (R.nty == 1 ? R.s0 : 0);
    R.n_first = R.nty == 1 ? R.n_last : slabs_per_tile(g) - R.s0;
    R.row_pitch = row_pitch;
    return region_valid(g, R);
}

// 64-row slabs of the region's tile rows, top to bottom
AQZ_HD inline uint64_t
region_slab_rows(const Geom& g, const Region& R)
{
    if (R.nty == 1)
        return R.n_first;
    return uint64_t(R.n_first) + uint64_t(R.nty - 2) * slabs_per_tile(g) + R.n_last;
}

// work items of one frame of the region: (slab row, tile column), the tile
// column fastest
AQZ_HD inline uint64_t
region_items_per_frame(const Geom& g, const Region& R)
{
    return region_slab_rows(g, R) * R.ntx;
}

// tile_rect's rectangle clipped to the region; the destination is relative
// to the crop's first byte.  kMove only when every source byte lies inside
// [0, bpc) of a chunk below n_chunks and every destination byte inside the
// width * bpp bytes of a row below height of the crop.
AQZ_HD inline uint32_t
region_rect(const Geom& g, const Region& R, uint32_t grp, uint64_t internal, uint32_t ty,
            uint32_t tx, uint32_t slab, Rect& r)
{
    const uint32_t st = tile_rect(g, grp, internal, ty, tx, slab, r);
    if (st != kMove)
        return st;
    if (R.row_pitch < uint64_t(region_width(g, R)) * g.bpp)
        return kBad;
    const uint64_t Y0 = uint64_t(ty) * g.th + uint64_t(slab) * kSlabRows;
    const uint64_t X0 = uint64_t(tx) * g.tw;
    const uint64_t ya = Y0 > R.y0 ? Y0 : R.y0, xa = X0 > R.x0 ? X0 : R.x0;
    uint64_t yb = Y0 + r.rows, xb = X0 + r.cols;
    if (yb > uint64_t(R.y0) + R.h)
        yb = uint64_t(R.y0) + R.h;
    if (xb > uint64_t(R.x0) + R.w)
        xb = uint64_t(R.x0) + R.w;
    if (yb <= ya || xb <= xa)
        return kEmpty;
    const uint64_t rows = yb - ya, cols = xb - xa;
    r.src += (ya - Y0) * r.src_pitch + (xa - X0) * g.bpp;
    r.rows = uint32_t(rows);
    r.cols = uint32_t(cols);
    if (r.src + (rows - 1) * r.src_pitch + cols * g.bpp > g.bpc)
        return kBad;
    const uint64_t ry = ya - R.y0, rx = xa - R.x0; // inside the region
    if (ry + rows > R.h || rx + cols > R.w)
        return kBad;
    r.dst_pitch = R.row_pitch;
    if (!g.xy) {
        r.dst = ry * R.row_pitch + rx * g.bpp;
        r.dst_rows = r.rows;
        r.dst_row_bytes = cols * g.bpp;
    } else {
        // storage pixel (y, x) -> row x, pixel y of a crop of R.w rows of R.h
        r.dst = rx * R.row_pitch + ry * g.bpp;
        r.dst_rows = r.cols;
        r.dst_row_bytes = rows * g.bpp;
    }
    if (r.dst + (uint64_t(r.dst_rows) - 1) * r.dst_pitch + r.dst_row_bytes >
        region_frame_extent(g, R))
        return kBad;
    return kMove;
}

// (ty, slab) of slab row `j` (< region_slab_rows) of the region
AQZ_HD inline void
region_slab_row(const Geom& g, const Region& R, uint64_t j, uint32_t& ty, uint32_t& slab)
{
    if (j < R.n_first) {
        ty = R.ty0;
        slab = R.s0 + uint32_t(j);
        return;
    }
    const uint64_t k = j - R.n_first;
    const uint32_t spt = slabs_per_tile(g);
    ty = R.ty0 + 1 + uint32_t(k / spt);
    slab = uint32_t(k % spt);
}

// Work item `item` (< region_items_per_frame) of layer-local frame `frame`,
// as unsplit_item: the mover holds the source and the crop of that frame.
template<bool XY, class Mover>
AQZ_HD inline uint32_t
region_item(const Geom& g, const Region& R, const uint32_t* tab_grp, const uint64_t* tab_off,
            const uint64_t* chunk_src, uint32_t frame, uint64_t item, Mover& m)
{
    // R is make_region's (the launch checks region_valid on the host); whatever
    // it holds, region_rect bounds every byte by itself
    if (frame >= g.n_frames || XY != (g.xy != 0) || R.ntx == 0 || g.th == 0 ||
        item >= region_items_per_frame(g, R))
        return kBad;
    uint32_t ty, slab;
    region_slab_row(g, R, item / R.ntx, ty, slab);
    const uint32_t tx = R.tx0 + uint32_t(item % R.ntx);
    Rect r;
    const uint32_t st = region_rect(g, R, tab_grp[frame], tab_off[frame], ty, tx, slab, r);
    if (st != kMove)
        return st;
    const uint64_t base = chunk_src[r.chunk];
    if (base == kNoChunk)
        m.zero(r);
    else if constexpr (XY)
        m.transpose(base, r);
    else
        m.copy(base, r);
    return kMove;
}

// Host: mark[c] = 1 for every chunk that a read of frames [first, first +
// count) of the region can touch -- the tile ranges of the walk above, so a
// chunk the map can reach is always marked.  False when a chunk index leaves
// the layer (geometry and table disagree).
inline bool
region_mark_chunks(const Geom& g, const Region& R, uint32_t grp, uint8_t* mark)
{
    for (uint32_t ty = R.ty0; ty < R.ty0 + R.nty; ++ty)
        for (uint32_t tx = R.tx0; tx < R.tx0 + R.ntx; ++tx) {
            const uint64_t c = uint64_t(grp) + uint64_t(ty) * g.ntx + tx;
            if (c >= g.n_chunks)
                return false;
            mark[c] = 1;
        }
    return true;
}

// Host: the byte hull of the region inside every chunk a read of one frame
// touches -- lo[c] falls to the first and hi[c] rises to one past the last
// chunk byte of the rectangles region_item hands to the mover (start lo at
// ~0 and hi at 0; a chunk the frame does not touch keeps both).  The walk is
// region_item's own, so a decoder that produced only [lo[c], hi[c]) of chunk
// c has produced every byte the crop reads.  False when the map refuses a
// rectangle (geometry and table disagree).
inline bool
region_hull_frame(const Geom& g, const Region& R, uint32_t grp, uint64_t internal, uint64_t* lo,
                  uint64_t* hi)
{
    const uint64_t slab_rows = region_slab_rows(g, R);
    for (uint64_t j = 0; j < slab_rows; ++j) {
        uint32_t ty, slab;
        region_slab_row(g, R, j, ty, slab);
        for (uint32_t tx = R.tx0; tx < R.tx0 + R.ntx; ++tx) {
            Rect r;
            const uint32_t st = region_rect(g, R, grp, internal, ty, tx, slab, r);
            if (st == kBad)
                return false;
            if (st != kMove)
                continue;
            const uint64_t a = r.src;
            const uint64_t b = r.src + (uint64_t(r.rows) - 1) * r.src_pitch + uint64_t(r.cols) * g.bpp;
            if (a < lo[r.chunk])
                lo[r.chunk] = a;
            if (b > hi[r.chunk])
                hi[r.chunk] = b;
        }
    }
    return true;
}

// copy_unit for a crop: the clip edges x0 and x0 + w and the crop's row pitch
// join the word; the frame's own row length does not (a rectangle is cut
// either at a tile edge or at a region edge).  `align` also holds the
// destination address and the destination frame stride.
inline uint32_t
region_copy_unit(const Geom& g, const Region& R, uint64_t align)
{
    const uint64_t a = align | uint64_t(g.tw) * g.bpp | uint64_t(R.x0) * g.bpp |
                       uint64_t(R.w) * g.bpp | R.row_pitch | 16u;
    return uint32_t(a & (~a + 1));
}

// XY path of a crop: may pixels be moved as words of bpp bytes?
inline bool
region_pixel_aligned(const Geom& g, const Region& R, uint64_t align)
{
    return pixel_aligned(g, align | R.row_pitch);
}

// One launch: the crop of frames [first, first + count) -> p.dst + i *
// p.dst_stride, rows at r.row_pitch; p.dst_stride >= region_frame_extent
struct RegionParams
{
    Params p;
    Region r;
};

} // namespace unsplit
} // namespace aqz
