// aqz_decode.hh -- device decoder of blosc1 frames with the LZ4 codec (and
// memcpyed frames): the inverse of aqz_codec.hh's blosc-lz4 row, for any
// conforming frame (this library's 4 KiB streams or c-blosc's, any block
// size, split or not, all three shuffle modes).  The parse and every bound
// live in aqz_lz4dec.hh, shared with the host.
//
// A malformed frame is a status in status[], never a fault: reads end at
// the frame's end, writes at the stream's end, and a bad frame stops only
// its own workgroups.
#pragma once

#include "aqz_lz4dec.hh"

#include <hip/hip_runtime.h>

#include <cstdint>

namespace aqz {

// Bytes of decoded (still shuffled) blocks a workgroup keeps in LDS.  Frames
// whose block size is at most this decode and un-shuffle without touching
// global scratch (always true of this library's own frames: 4 KiB streams,
// typesize <= 8); larger blocks decode into DecodeParams::scratch and a
// second kernel un-shuffles them.
constexpr uint32_t kDecodeLdsBytes = 32 * 1024;

struct DecodeParams
{
    const uint8_t* frames;   // n_chunks frames back to back
    uint64_t frames_bytes;
    const uint64_t* offsets; // [n_chunks + 1] frame starts + total (device)
    uint32_t n_chunks;
    uint8_t* dst;            // frame q -> dst + slot(q) * pitch
    uint64_t pitch;
    uint64_t chunk_bytes;
    uint32_t* status;        // [n_chunks] dec::k* per frame (by position q)
    const uint32_t* order;   // slot(q) = order[q]; nullptr: q
    // compare mode (bad != nullptr): dst is not written; bad[q] becomes 1
    // when the decoded bytes differ from the chunk at dst (a zero-length
    // frame: when that chunk is not all zero)
    uint32_t* bad;
    uint8_t* scratch;        // n_chunks * scratch_pitch bytes; nullptr: frames
                             // with blocks above kDecodeLdsBytes are kUnsupported
    uint64_t scratch_pitch;  // >= chunk_bytes, a multiple of 16
    // codec families of the run (dec::kFamily*); 0 = kFamilyLz4.  Frames of a
    // family that is not listed get kUnsupported; with kFamilyZstd listed,
    // launch_blosc_decode leaves zstd frames to launch_zstd_decode
    // (aqz_zstddec.hip), which runs behind it on the same stream.
    uint32_t codecs;
    // launch_zstd_decode only: Huffman literals of the block a workgroup
    // decodes, zlit_pitch bytes per (chunk, pass), zpasses passes per chunk.
    // scratch must be set (staging of shuffled blocks and of compare mode).
    uint8_t* zlit;
    uint64_t zlit_pitch;
    uint32_t zpasses;
    // launch_zstd_parallel only (aqz_zstdpar.hip); zfr == nullptr: not in use.
    // zfr[2q]: 0 = frame q is zstd_decode's, else 1 + the blocks indexed (the
    // frame is the parallel kernels'); zfr[2q + 1]: its sequences.  zcounts:
    // the four words of aqz_decode_counts.  zpar: per chunk (zpar_pitch) the
    // block table, the literal area and the records (zstd_parallel_layout).
    uint32_t* zfr;
    uint32_t* zcounts;
    uint8_t* zpar;
    uint64_t zpar_pitch, zpar_lit_off, zpar_rec_off;
    uint32_t zpar_cap;
};

// Enqueue: status (and bad) cleared, frames decoded, large blocks un-shuffled.
hipError_t launch_blosc_decode(const DecodeParams& p, hipStream_t stream);

// Passes per chunk and literal bytes per pass launch_zstd_decode needs for
// chunks of up to max_chunk_bytes.
constexpr uint32_t kZstdMaxPasses = 8;
uint32_t zstd_decode_passes(uint64_t max_chunk_bytes);
uint64_t zstd_decode_lit_pitch(uint64_t max_chunk_bytes);
// Enqueue behind launch_blosc_decode (which cleared status and bad): the
// run's zstd frames -- plain zstd, blosc1 with the zstd codec (memcpyed ones
// included) -- decoded; other frames are not touched.
hipError_t launch_zstd_decode(const DecodeParams& p, hipStream_t stream);

// ---- ranged decode: only the blosc blocks that meet a byte range ----------
// A run of DecodeParams p (no compare mode) in which frame q is decoded over
// chunk bytes ranges[q] only (dec::range_status, dec::blocks_of_range):
//   blosc1 frames      only the blocks that meet the range are looked up in
//                      bstarts, decoded and un-shuffled; the span is the
//                      block-aligned interval of dec::blocks_of_range
//   memcpyed frames,   only [lo, hi) is copied / zero-filled; the span is
//   zero-length frames [lo, hi)
//   plain zstd frames  decoded whole (matches reach across blocks); the span
//                      is [0, chunk_bytes)
//   an empty range     status dec::kNotLoaded, empty span, the frame is not
//                      decoded; a reversed range or hi > chunk_bytes:
//                      dec::kBadHeader, empty span
// No byte of a chunk outside its span is written.
struct RangedParams
{
    DecodeParams p;
    const dec::ByteRange* ranges; // [n_chunks] by frame position (device)
    dec::ByteRange* spans;        // [n_chunks] what was decoded; nullptr: not wanted
};
// Enqueue: status and spans cleared; the LZ4, memcpyed and zero-length frames
// decoded over their ranges and the statuses of empty and bad ranges set for
// frames of every family.  max_range_bytes: an upper bound of hi - lo over
// the run that sizes the grid (the needed blocks of a chunk are dealt over
// the workgroups by their own count); 0 = unknown, chunk_bytes.
hipError_t launch_blosc_decode_ranged(const RangedParams& rp, uint64_t max_range_bytes,
                                      hipStream_t stream);
// Enqueue behind it (and behind launch_zstd_parallel, where in use): the zstd
// frames of the run, as launch_zstd_decode.
hipError_t launch_zstd_decode_ranged(const RangedParams& rp, uint64_t max_range_bytes,
                                     hipStream_t stream);

// The block-parallel path of plain zstd frames (AQZ_DECODE_ZSTD_PARALLEL).
// Per chunk of up to max_chunk_bytes: a table of cap blocks, then the literal
// area, then the records; pitch bytes in all.
struct ZstdParLayout
{
    uint64_t lit_off, rec_off, pitch;
    uint32_t cap;
};
ZstdParLayout zstd_parallel_layout(uint64_t max_chunk_bytes);
// Device bytes the path adds: the chunks' slots, two words per chunk and the
// four count words.
uint64_t zstd_parallel_bytes(uint64_t max_chunk_bytes, uint32_t max_chunks);
// Enqueue between launch_blosc_decode and launch_zstd_decode: the plain zstd
// frames whose blocks fit the table are decoded (or get their status) and
// marked in zfr; zstd_decode then skips them, zstd_finish does not.
hipError_t launch_zstd_parallel(const DecodeParams& p, hipStream_t stream);

} // namespace aqz
