// aqz_reader.hh -- the device reader: one level's chunk layers back to
// row-major frames in device memory.
//
//   Reader <- the inverse of zarr::Array::write_frame_to_chunks_
//             (src/streaming/array.cpp:537-619) and, through the device
//             decoders, of Array::compress_and_flush_data_ (array.cpp:
//             777-803).  The reference has no read path.
#pragma once

#include "aqz_engine.hh"
#include "aqz_region.hh"
#include "aqz_unsplit.hh"

namespace aqz {

// aqz_unsplit.hip.  align: see unsplit::copy_unit.
hipError_t launch_unsplit(const unsplit::Params& p, uint64_t align, hipStream_t stream);
// the crop of q.r; align as above plus the destination's frame stride
hipError_t launch_unsplit_region(const unsplit::RegionParams& q, uint64_t align,
                                 hipStream_t stream);
hipError_t launch_chunk_table(uint64_t* chunk_src, uint32_t n, uint64_t pitch,
                              const uint32_t* has_data, uint32_t tag, hipStream_t stream);

struct ReaderDesc
{
    std::vector<Dim> dims; // of this level, acquisition order
    int32_t dtype = 0;
    std::vector<size_t> storage_order; // level 0 only
    uint32_t codecs = 0;               // dec::kFamily*; 0 = raw chunks only
    uint64_t max_frames_bytes = 0;     // 0 = Compressor::max_bytes of a layer
    int32_t device = 0;
};

class Reader
{
  public:
    explicit Reader(const ReaderDesc& d);
    ~Reader();
    Reader(const Reader&) = delete;
    Reader& operator=(const Reader&) = delete;

    // device bytes Reader(d) allocates, exactly; 0 for an invalid description.
    // Needs no GPU.
    static uint64_t device_bytes_for(const ReaderDesc& d);
    uint64_t device_bytes() const;
    LevelLayout layout() const;
    int device() const { return device_; }

    // codec: 0 none, 1 blosc-lz4, 2 blosc-zstd, 3 zstd (Compression::codec)
    void load_frames(const void* frames, size_t frames_bytes, int mem, const uint64_t* offsets,
                     const uint32_t* chunk_of_frame, uint32_t n_frames, int32_t codec,
                     hipStream_t stream);
    // load_frames for the window (first, count, region) only: frames of other
    // chunks are neither copied nor decoded, and their bytes are not read
    void load_frames_region(const void* frames, size_t frames_bytes, int mem,
                            const uint64_t* offsets, const uint32_t* chunk_of_frame,
                            uint32_t n_frames, int32_t codec, uint32_t first, uint32_t count,
                            const RegionArg* region, hipStream_t stream);
    // load_frames_region, decoding each chunk of the window over the window's
    // byte hull only (region_chunk_ranges); chunks outside the window are
    // neither decoded nor zero-filled, and reads are held to the exact window.
    // The first call allocates 32 bytes per chunk (device and pinned): the
    // ranges given to the decoder and the spans it reports.
    void load_frames_window(const void* frames, size_t frames_bytes, int mem,
                            const uint64_t* offsets, const uint32_t* chunk_of_frame,
                            uint32_t n_frames, int32_t codec, uint32_t first, uint32_t count,
                            const RegionArg* region, hipStream_t stream);
    void load_chunks(const void* chunks, uint64_t pitch, const uint32_t* has_data, uint32_t tag,
                     hipStream_t stream);
    void read_frames(uint32_t first, uint32_t count, void* dst, uint64_t dst_stride,
                     hipStream_t stream);
    // the crop of frames [first, first + count): pixel (y0 + j, x0 + i) of frame
    // first + k -> dst + k * dst_frame_stride + j * dst_row_stride + i * bpp
    void read_region(uint32_t first, uint32_t count, const RegionArg* region, void* dst,
                     uint64_t dst_row_stride, uint64_t dst_frame_stride, hipStream_t stream);
    std::vector<uint32_t> region_chunks(uint32_t first, uint32_t count,
                                        const RegionArg* region) const;
    std::vector<ChunkRange> region_chunk_ranges(uint32_t first, uint32_t count,
                                                const RegionArg* region) const;
    // waits for the last load; status[c] of chunk c, *n_bad = error statuses
    void status(uint32_t* status, size_t cap, uint32_t* n_bad);
    // waits for the last load.  decoded: chunk bytes its decoder wrote (decoded,
    // copied out of memcpyed frames or zero-filled; the sum of the spans of a
    // window load; 0 without a decoder); copied: frame bytes it copied into
    // the staging buffer.
    void load_stats(uint64_t* decoded, uint64_t* copied);

  private:
    struct Sizes;
    static Sizes sizes(const ReaderDesc& d, const ArrayDimensions& ad);
    void begin_load(hipStream_t stream);
    // window: per chunk, 1 = inside the loaded window; nullptr = the whole layer.
    // hull (with a window): the decoder runs over these byte ranges of the
    // window's chunks, and over nothing of the others.
    void load(const void* frames, size_t frames_bytes, int mem, const uint64_t* offsets,
              const uint32_t* chunk_of_frame, uint32_t n_frames, int32_t codec,
              const uint8_t* window, const std::vector<ChunkRange>* hull, hipStream_t stream);
    // a read of these frames of this region stays inside the loaded window;
    // `region` in acquisition orientation, as the caller gave it
    void check_window(uint32_t first, uint32_t count, const unsplit::Region& R,
                      const RegionArg& region) const;
    [[noreturn]] void refuse_read(const std::string& what) const;

    int32_t device_;
    uint32_t codecs_;
    std::unique_ptr<ArrayDimensions> ad_;
    unsplit::Geom g_{};
    std::vector<uint32_t> shard_order_; // position -> chunk, as compress_layer writes
    std::vector<uint32_t> h_tab_grp_;   // host copy of tab_grp: the chunk sets of regions
    // one device block: [tab_off F u64][chunk_src n u64][offsets n+1 u64]
    // [tab_grp F u32][order n u32][status n u32]
    DevBuf tables_;
    uint64_t* d_tab_off_ = nullptr;
    uint64_t* d_chunk_src_ = nullptr;
    uint64_t* d_offsets_ = nullptr;
    uint32_t* d_tab_grp_ = nullptr;
    uint32_t* d_order_ = nullptr;
    uint32_t* d_status_ = nullptr;
    // pinned mirror of the per-load part: [chunk_src n][offsets n+1][order n][status n]
    PinnedBuf h_words_;
    uint64_t* h_chunk_src_ = nullptr;
    uint64_t* h_offsets_ = nullptr;
    uint32_t* h_order_ = nullptr;
    uint32_t* h_status_ = nullptr;
    DevBuf layer_;  // decoded chunks at layer_pitch_ (codecs != 0)
    uint64_t layer_pitch_ = 0;
    DevBuf staging_; // frames that arrive from host memory
    std::unique_ptr<Decompressor> dec_;
    // the loaded layer
    enum class Loaded
    {
        None,
        Decoded, // status words come from the decoder, by frame position
        Raw,     // status words were set on the host, by chunk
        Chunks   // chunk_src was made on the device and copied back
    } loaded_ = Loaded::None;
    uint32_t loaded_frames_ = 0;
    const uint8_t* src_ = nullptr;
    uint64_t src_align_ = 0;
    std::vector<uint32_t> chunk_status_;
    // the window of the last load_frames_region (host memory only): the chunks
    // it loaded, and its description for the error text
    bool windowed_ = false;
    // the window came from load_frames_window: only its hull was decoded, so a
    // read has to stay inside its frames and its region, not just its chunks
    bool window_exact_ = false;
    // load_frames_window's words, allocated by its first call: device
    // [ranges n][spans n], and their pinned mirror
    DevBuf d_ranges_;
    PinnedBuf h_ranges_;
    bool ranged_ = false;       // the last load ran the decoder over ranges
    uint64_t stat_decoded_ = 0; // of the last load (not ranged_)
    uint64_t stat_copied_ = 0;
    std::vector<uint8_t> window_;
    uint32_t window_first_ = 0, window_count_ = 0;
    RegionArg window_region_{};
    hipEvent_t load_ev_ = nullptr; // the last load has run
    hipEvent_t read_ev_ = nullptr; // the last read has run
    bool read_pending_ = false;
};

} // namespace aqz
