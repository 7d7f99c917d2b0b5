// aqz_reader.cpp -- see aqz_reader.hh.  Citations are to the reference's
// src/streaming/.
#include "aqz_reader.hh"

#include <algorithm>
#include <cstring>
#include <string>

namespace aqz {

namespace {

constexpr int kMemHost = 0, kMemDevice = 1, kMemHostPinned = 2;
// AQZ_DECODE_NOT_LOADED: a chunk outside the window of a region load
constexpr uint32_t kNotLoaded = 5;

uint64_t
round16(uint64_t n)
{
    return (n + 15) & ~uint64_t(15);
}

// dec::kFamily* a Compression::codec value needs (0: none; ~0u: no such codec)
uint32_t
family_of(int32_t codec)
{
    switch (codec) {
        case 0: return 0;
        case 1: return dec::kFamilyLz4;
        case 2:
        case 3: return dec::kFamilyZstd;
        default: return ~0u;
    }
}

} // namespace

struct Reader::Sizes
{
    uint32_t F = 0, n = 0;
    uint64_t tables = 0, words = 0, layer_pitch = 0, layer = 0, staging = 0, decoder = 0;
};

Reader::Sizes
Reader::sizes(const ReaderDesc& d, const ArrayDimensions& ad)
{
    if (d.codecs && !decode_codecs_valid(d.codecs))
        throw Error(1, "codecs: AQZ_DECODE_CODEC_LZ4 | AQZ_DECODE_CODEC_ZSTD, or 0; "
                       "AQZ_DECODE_ZSTD_PARALLEL only with the latter alone");
    Sizes s;
    const uint64_t F = ad.frames_per_chunk_layer();
    if (F == 0 || F > 0x7fffffffull)
        throw Error(9, "unsupported frames per chunk layer");
    const uint64_t bpc = ad.bytes_per_chunk();
    if (bpc == 0 || bpc > 0x7fffffefull)
        throw Error(9, "chunk size outside the blosc1 limits");
    const uint64_t tile_row = uint64_t(ad.width_dim().chunk_size_px) * bytes_of_type(d.dtype);
    if (tile_row * unsplit::kSlabRows > 0xffffffffull)
        throw Error(9, "tile rows too long");
    if (ad.width_dim().array_size_px == 0 || ad.height_dim().array_size_px == 0)
        throw Error(9, "frame dimensions must be bounded");
    s.F = uint32_t(F);
    s.n = ad.number_of_chunks_in_memory();
    if (s.n == 0)
        throw Error(9, "no chunks");
    s.words = uint64_t(s.n) * 8 + (uint64_t(s.n) + 1) * 8 + uint64_t(s.n) * 4 * 2;
    s.tables = uint64_t(s.F) * 12 + s.words;
    if (d.codecs) {
        s.layer_pitch = round16(bpc);
        s.layer = s.layer_pitch * s.n;
        s.decoder = Decompressor::scratch_bytes(bpc, s.n, true, d.codecs);
    }
    s.staging = d.max_frames_bytes ? d.max_frames_bytes : Compressor::max_bytes(bpc, s.n);
    return s;
}

uint64_t
Reader::device_bytes_for(const ReaderDesc& d)
{
    try {
        const ArrayDimensions ad(d.dims, d.dtype, d.storage_order);
        const Sizes s = sizes(d, ad);
        return s.tables + s.layer + s.staging + s.decoder;
    } catch (const std::exception&) {
        return 0;
    }
}

Reader::Reader(const ReaderDesc& d)
  : device_(d.device)
  , codecs_(d.codecs)
{
    ad_ = std::make_unique<ArrayDimensions>(d.dims, d.dtype, d.storage_order);
    const Sizes s = sizes(d, *ad_);
    g_ = unsplit_geom(*ad_);

    // the stage's per-frame tables (aqz_engine.cpp, Stage::Stage), with the
    // chunk's own offset instead of a ring pitch folded in
    std::vector<uint64_t> tab_off(s.F);
    std::vector<uint32_t>& tab_grp = h_tab_grp_;
    tab_grp.resize(s.F);
    for (uint32_t f = 0; f < s.F; ++f) {
        const uint64_t sf = ad_->transpose_frame_id(f);
        tab_grp[f] = ad_->tile_group_offset(sf);
        tab_off[f] = ad_->chunk_internal_offset(sf);
    }
    {
        std::vector<uint32_t> shard, internal0;
        shard_major_order(*ad_, shard_order_, shard, internal0);
    }
    chunk_status_.assign(s.n, dec::kSkipped);

    hip_check(hipSetDevice(device_), "hipSetDevice");
    tables_.alloc(s.tables);
    uint8_t* q = tables_.p;
    d_tab_off_ = reinterpret_cast<uint64_t*>(q);
    q += size_t(s.F) * 8;
    d_chunk_src_ = reinterpret_cast<uint64_t*>(q);
    q += size_t(s.n) * 8;
    d_offsets_ = reinterpret_cast<uint64_t*>(q);
    q += (size_t(s.n) + 1) * 8;
    d_tab_grp_ = reinterpret_cast<uint32_t*>(q);
    q += size_t(s.F) * 4;
    d_order_ = reinterpret_cast<uint32_t*>(q);
    q += size_t(s.n) * 4;
    d_status_ = reinterpret_cast<uint32_t*>(q);
    hip_check(hipMemcpy(d_tab_off_, tab_off.data(), size_t(s.F) * 8, hipMemcpyHostToDevice),
              "hipMemcpy");
    hip_check(hipMemcpy(d_tab_grp_, tab_grp.data(), size_t(s.F) * 4, hipMemcpyHostToDevice),
              "hipMemcpy");
    h_words_.alloc(s.words);
    uint8_t* h = h_words_.p;
    h_chunk_src_ = reinterpret_cast<uint64_t*>(h);
    h += size_t(s.n) * 8;
    h_offsets_ = reinterpret_cast<uint64_t*>(h);
    h += (size_t(s.n) + 1) * 8;
    h_order_ = reinterpret_cast<uint32_t*>(h);
    h += size_t(s.n) * 4;
    h_status_ = reinterpret_cast<uint32_t*>(h);
    if (codecs_) {
        layer_pitch_ = s.layer_pitch;
        layer_.alloc(s.layer);
        dec_ = std::make_unique<Decompressor>(g_.bpc, s.n, true, codecs_);
    }
    staging_.alloc(s.staging);
    hip_check(hipEventCreateWithFlags(&load_ev_, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventCreateWithFlags(&read_ev_, hipEventDisableTiming), "hipEventCreate");
}

Reader::~Reader()
{
    // a borrowed source or destination may still be in use by enqueued work
    if (load_ev_) {
        (void)hipEventSynchronize(load_ev_);
        (void)hipEventDestroy(load_ev_);
    }
    if (read_ev_) {
        (void)hipEventSynchronize(read_ev_);
        (void)hipEventDestroy(read_ev_);
    }
    (void)hipGetLastError();
}

uint64_t
Reader::device_bytes() const
{
    return tables_.n + layer_.n + staging_.n + d_ranges_.n + (dec_ ? dec_->device_bytes() : 0);
}

LevelLayout
Reader::layout() const
{
    LevelLayout l{};
    l.bytes_per_chunk = g_.bpc;
    l.chunks_per_layer = g_.n_chunks;
    l.layer_slots = 1;
    l.frames_per_layer = g_.n_frames;
    l.frame_bytes = unsplit::frame_bytes(g_);
    // of the frames handed back: acquisition orientation
    l.width = g_.xy ? g_.H : g_.W;
    l.height = g_.xy ? g_.W : g_.H;
    l.chunk_pitch = layer_pitch_ ? layer_pitch_ : g_.bpc;
    return l;
}

// The pinned words and the layer buffer are about to be rewritten: the
// previous load's copies have to be done (host side), and the reads of the
// previous layer enqueued so far have to run first (device side).
void
Reader::begin_load(hipStream_t stream)
{
    if (loaded_ != Loaded::None)
        hip_check(hipEventSynchronize(load_ev_), "hipEventSynchronize");
    if (read_pending_)
        hip_check(hipStreamWaitEvent(stream, read_ev_, 0), "hipStreamWaitEvent");
    loaded_ = Loaded::None;
}

void
Reader::load_frames(const void* frames, size_t frames_bytes, int mem, const uint64_t* offsets,
                    const uint32_t* chunk_of_frame, uint32_t n_frames, int32_t codec,
                    hipStream_t stream)
{
    load(frames, frames_bytes, mem, offsets, chunk_of_frame, n_frames, codec, nullptr, nullptr,
         stream);
    windowed_ = false;
    window_exact_ = false;
}

void
Reader::load_frames_region(const void* frames, size_t frames_bytes, int mem,
                           const uint64_t* offsets, const uint32_t* chunk_of_frame,
                           uint32_t n_frames, int32_t codec, uint32_t first, uint32_t count,
                           const RegionArg* region, hipStream_t stream)
{
    std::vector<uint8_t> window(g_.n_chunks, 0);
    for (uint32_t c : region_chunks(first, count, region))
        window[c] = 1;
    load(frames, frames_bytes, mem, offsets, chunk_of_frame, n_frames, codec, window.data(),
         nullptr, stream);
    window_.swap(window);
    window_first_ = first;
    window_count_ = count;
    window_region_ = *region;
    windowed_ = true;
    window_exact_ = false;
}

void
Reader::load_frames_window(const void* frames, size_t frames_bytes, int mem,
                           const uint64_t* offsets, const uint32_t* chunk_of_frame,
                           uint32_t n_frames, int32_t codec, uint32_t first, uint32_t count,
                           const RegionArg* region, hipStream_t stream)
{
    const std::vector<ChunkRange> hull = region_chunk_ranges(first, count, region);
    std::vector<uint8_t> window(g_.n_chunks, 0);
    for (const ChunkRange& c : hull)
        window[c.chunk] = 1;
    if (!d_ranges_.p && codecs_) {
        d_ranges_.alloc(size_t(g_.n_chunks) * 2 * sizeof(dec::ByteRange));
        h_ranges_.alloc(size_t(g_.n_chunks) * 2 * sizeof(dec::ByteRange));
    }
    load(frames, frames_bytes, mem, offsets, chunk_of_frame, n_frames, codec, window.data(),
         &hull, stream);
    window_.swap(window);
    window_first_ = first;
    window_count_ = count;
    window_region_ = *region;
    windowed_ = true;
    window_exact_ = true;
}

// With a window, the frames of chunks outside it are dropped here: they take
// no decoder position of their own, nothing of them is copied and their bytes
// are never addressed.  The frames that are needed are packed back to back
// into the staging buffer (runs of adjacent frames in one copy each) whenever
// the decoder runs or the frames lie in host memory; stored chunks in device
// memory are borrowed where they lie.
void
Reader::load(const void* frames, size_t frames_bytes, int mem, const uint64_t* offsets,
             const uint32_t* chunk_of_frame, uint32_t n_frames, int32_t codec,
             const uint8_t* window, const std::vector<ChunkRange>* hull, hipStream_t stream)
{
    const uint32_t n = g_.n_chunks;
    const uint32_t fam = family_of(codec);
    if (fam == ~0u)
        throw Error(1, "unknown codec");
    if (fam && !(codecs_ & fam))
        throw Error(1, "the reader was not created for this codec");
    if (!offsets || (!frames && frames_bytes))
        throw Error(1, "null frames or offsets");
    if (mem != kMemHost && mem != kMemDevice && mem != kMemHostPinned)
        throw Error(1, "mem: AQZ_MEM_HOST, AQZ_MEM_HOST_PINNED or AQZ_MEM_DEVICE");
    if (n_frames > n)
        throw Error(1, "more frames than chunks per layer");
    if (!chunk_of_frame && n_frames != n)
        throw Error(1, "without chunk_of_frame every chunk of the layer has a frame");
    if (offsets[0] > frames_bytes)
        throw Error(1, "offsets exceed frames_bytes");
    for (uint32_t q = 0; q < n_frames; ++q)
        if (offsets[q + 1] < offsets[q] || offsets[q + 1] > frames_bytes)
            throw Error(1, "offsets are not monotonic or exceed frames_bytes");
    const uint32_t* order = chunk_of_frame ? chunk_of_frame : shard_order_.data();
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t q = 0; q < n_frames; ++q) {
        if (order[q] >= n)
            throw Error(1, "chunk_of_frame entry outside the layer");
        if (seen[order[q]])
            throw Error(1, "chunk_of_frame lists a chunk twice");
        seen[order[q]] = 1;
    }
    const bool pack = window && (mem != kMemDevice || fam);
    if (pack) {
        uint64_t needed = 0;
        for (uint32_t q = 0; q < n_frames; ++q)
            if (window[order[q]])
                needed += offsets[q + 1] - offsets[q];
        if (needed > staging_.n)
            throw Error(1, mem == kMemDevice
                             ? "the needed frames' bytes above the reader's max_frames_bytes "
                               "(compressed frames in device memory are packed into the "
                               "staging buffer for a region load too)"
                             : "the needed frames' bytes above the reader's max_frames_bytes");
    } else if (mem != kMemDevice && frames_bytes > staging_.n) {
        throw Error(1, "frames_bytes above the reader's max_frames_bytes");
    }

    begin_load(stream);
    const uint8_t* given = static_cast<const uint8_t*>(frames);
    const uint8_t* dframes = given;
    if (pack) {
        dframes = staging_.p;
    } else if (mem != kMemDevice) {
        if (frames_bytes)
            hip_check(hipMemcpyAsync(staging_.p, frames, frames_bytes, hipMemcpyHostToDevice,
                                     stream),
                      "hipMemcpyAsync");
        dframes = staging_.p;
    }
    for (uint32_t c = 0; c < n; ++c)
        h_chunk_src_[c] = unsplit::kNoChunk;
    std::fill(chunk_status_.begin(), chunk_status_.end(), uint32_t(dec::kSkipped));
    // the pending copy of a run of adjacent needed frames (pack only)
    const hipMemcpyKind kind =
      mem == kMemDevice ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint64_t run_src = 0, run_dst = 0, run_len = 0, packed = 0;
    auto flush = [&] {
        if (run_len)
            hip_check(hipMemcpyAsync(staging_.p + run_dst, given + run_src, run_len, kind,
                                     stream),
                      "hipMemcpyAsync");
        run_len = 0;
    };
    uint64_t align = 0;
    uint32_t slot = 0; // decoder positions taken so far; q itself without a window
    for (uint32_t q = 0; q < n_frames; ++q) {
        const uint64_t len = offsets[q + 1] - offsets[q];
        const uint32_t c = order[q];
        if (window && !window[c]) {
            seen[c] = 0; // follows below as a zero-length frame, like a chunk not listed
            continue;
        }
        const uint64_t at = pack ? packed : offsets[q];
        h_offsets_[slot] = at;
        h_order_[slot++] = c;
        if (len == 0)
            continue;
        if (pack) {
            if (run_len && offsets[q] == run_src + run_len) {
                run_len += len;
            } else {
                flush();
                run_src = offsets[q];
                run_dst = packed;
                run_len = len;
            }
            packed += len;
        }
        if (fam) {
            h_chunk_src_[c] = c * layer_pitch_;
        } else if (len == g_.bpc) {
            // a stored chunk is its own frame
            h_chunk_src_[c] = at;
            align |= at;
            chunk_status_[c] = dec::kOk;
        } else {
            chunk_status_[c] = dec::kBadHeader;
        }
    }
    flush();
    // the decoder takes a permutation of the layer's chunks (a slot per frame
    // of the run): the chunks not listed follow as zero-length frames
    const uint64_t end = pack ? packed : offsets[n_frames];
    const uint64_t dec_bytes = pack ? packed : frames_bytes;
    uint32_t fill = slot;
    for (uint32_t c = 0; c < n && fill < n; ++c)
        if (!seen[c]) {
            h_offsets_[fill] = end;
            h_order_[fill++] = c;
        }
    h_offsets_[n] = end;
    // [chunk_src][offsets] lie back to back on both sides
    hip_check(hipMemcpyAsync(d_chunk_src_, h_chunk_src_, size_t(n) * 8 + (size_t(n) + 1) * 8,
                             hipMemcpyHostToDevice, stream),
              "hipMemcpyAsync");
    if (fam) {
        hip_check(hipMemcpyAsync(d_order_, h_order_, size_t(n) * 4, hipMemcpyHostToDevice,
                                 stream),
                  "hipMemcpyAsync");
        if (hull) {
            // by decoder position: the hull for a chunk of the window, nothing for the rest
            dec::ByteRange* h_ranges = reinterpret_cast<dec::ByteRange*>(h_ranges_.p);
            dec::ByteRange* d_ranges = reinterpret_cast<dec::ByteRange*>(d_ranges_.p);
            std::vector<dec::ByteRange> by_chunk(n, dec::ByteRange{ 0, 0 });
            uint64_t longest = 0;
            for (const ChunkRange& c : *hull) {
                by_chunk[c.chunk] = dec::ByteRange{ c.lo, c.hi };
                longest = std::max(longest, c.hi - c.lo);
            }
            for (uint32_t q = 0; q < n; ++q)
                h_ranges[q] = by_chunk[h_order_[q]];
            hip_check(hipMemcpyAsync(d_ranges, h_ranges, size_t(n) * sizeof(dec::ByteRange),
                                     hipMemcpyHostToDevice, stream),
                      "hipMemcpyAsync");
            dec_->run_ranges(dframes, dec_bytes, d_offsets_, n, layer_.p, layer_pitch_, g_.bpc,
                             d_ranges, d_ranges + n, d_status_, stream, d_order_, longest);
            hip_check(hipMemcpyAsync(h_ranges + n, d_ranges + n,
                                     size_t(n) * sizeof(dec::ByteRange), hipMemcpyDeviceToHost,
                                     stream),
                      "hipMemcpyAsync");
        } else {
            dec_->run(dframes, dec_bytes, d_offsets_, n, layer_.p, layer_pitch_, g_.bpc,
                      d_status_, stream, d_order_);
        }
        hip_check(hipMemcpyAsync(h_status_, d_status_, size_t(n) * 4, hipMemcpyDeviceToHost,
                                 stream),
                  "hipMemcpyAsync");
        src_ = layer_.p;
        src_align_ = uint64_t(reinterpret_cast<uintptr_t>(layer_.p)) | layer_pitch_;
    } else {
        src_ = dframes;
        src_align_ = uint64_t(reinterpret_cast<uintptr_t>(dframes)) | align;
    }
    hip_check(hipEventRecord(load_ev_, stream), "hipEventRecord");
    loaded_frames_ = n;
    loaded_ = fam ? Loaded::Decoded : Loaded::Raw;
    ranged_ = fam && hull;
    stat_decoded_ = fam ? uint64_t(n) * g_.bpc : 0;
    stat_copied_ = pack ? packed : mem != kMemDevice ? frames_bytes : 0;
}

void
Reader::load_chunks(const void* chunks, uint64_t pitch, const uint32_t* has_data, uint32_t tag,
                    hipStream_t stream)
{
    if (!chunks)
        throw Error(1, "null chunks");
    if (pitch < g_.bpc)
        throw Error(1, "chunk pitch below bytes_per_chunk");
    begin_load(stream);
    hip_check(launch_chunk_table(d_chunk_src_, g_.n_chunks, pitch, has_data, tag, stream),
              "chunk table launch");
    hip_check(hipMemcpyAsync(h_chunk_src_, d_chunk_src_, size_t(g_.n_chunks) * 8,
                             hipMemcpyDeviceToHost, stream),
              "hipMemcpyAsync");
    hip_check(hipEventRecord(load_ev_, stream), "hipEventRecord");
    src_ = static_cast<const uint8_t*>(chunks);
    src_align_ = uint64_t(reinterpret_cast<uintptr_t>(chunks)) | pitch;
    loaded_ = Loaded::Chunks;
    windowed_ = false;
    window_exact_ = false;
    ranged_ = false;
    stat_decoded_ = stat_copied_ = 0;
}

void
Reader::read_frames(uint32_t first, uint32_t count, void* dst, uint64_t dst_stride,
                    hipStream_t stream)
{
    if (loaded_ == Loaded::None)
        throw Error(1, "no layer loaded");
    if (uint64_t(first) + count > g_.n_frames)
        throw Error(1, "frame range outside the layer");
    if (count == 0)
        return;
    if (!dst)
        throw Error(1, "null destination");
    if (dst_stride < unsplit::frame_bytes(g_))
        throw Error(1, "dst_stride below the frame size");
    if (windowed_) {
        unsplit::Region whole;
        unsplit::make_region(g_, 0, 0, g_.xy ? g_.H : g_.W, g_.xy ? g_.W : g_.H,
                             uint64_t(g_.xy ? g_.H : g_.W) * g_.bpp, whole);
        check_window(first, count, whole,
                     RegionArg{ 0, 0, g_.xy ? g_.H : g_.W, g_.xy ? g_.W : g_.H });
    }
    unsplit::Params p{};
    p.g = g_;
    p.src = src_;
    p.chunk_src = d_chunk_src_;
    p.tab_grp = d_tab_grp_;
    p.tab_off = d_tab_off_;
    p.dst = static_cast<uint8_t*>(dst);
    p.dst_stride = dst_stride;
    p.first = first;
    p.count = count;
    // the load may have been enqueued on another stream
    hip_check(hipStreamWaitEvent(stream, load_ev_, 0), "hipStreamWaitEvent");
    const uint64_t align = src_align_ | uint64_t(reinterpret_cast<uintptr_t>(dst)) | dst_stride;
    hip_check(launch_unsplit(p, align, stream), "unsplit launch");
    hip_check(hipEventRecord(read_ev_, stream), "hipEventRecord");
    read_pending_ = true;
}

void
Reader::refuse_read(const std::string& what) const
{
    throw Error(1, what + ", outside the loaded window: frames [" +
                     std::to_string(window_first_) + ", " +
                     std::to_string(uint64_t(window_first_) + window_count_) + "), region x0 " +
                     std::to_string(window_region_.x0) + " y0 " +
                     std::to_string(window_region_.y0) + " width " +
                     std::to_string(window_region_.width) + " height " +
                     std::to_string(window_region_.height));
}

void
Reader::check_window(uint32_t first, uint32_t count, const unsplit::Region& R,
                     const RegionArg& region) const
{
    if (window_exact_) {
        // only the window's own bytes were decoded: the read stays inside its
        // frames and its region (sums in 64 bits; both regions are valid)
        const RegionArg& w = window_region_;
        if (first < window_first_ ||
            uint64_t(first) + count > uint64_t(window_first_) + window_count_)
            refuse_read("the read needs frames [" + std::to_string(first) + ", " +
                        std::to_string(uint64_t(first) + count) + ")");
        if (region.x0 < w.x0 || region.y0 < w.y0 ||
            uint64_t(region.x0) + region.width > uint64_t(w.x0) + w.width ||
            uint64_t(region.y0) + region.height > uint64_t(w.y0) + w.height)
            refuse_read("the read needs region x0 " + std::to_string(region.x0) + " y0 " +
                        std::to_string(region.y0) + " width " + std::to_string(region.width) +
                        " height " + std::to_string(region.height));
        return;
    }
    std::vector<uint8_t> mark(g_.n_chunks, 0);
    for (uint32_t f = first; f < first + count; ++f)
        if (!unsplit::region_mark_chunks(g_, R, h_tab_grp_[f], mark.data()))
            throw Error(9, "the frame tables leave the layer");
    for (uint32_t c = 0; c < g_.n_chunks; ++c)
        if (mark[c] && !window_[c])
            refuse_read("the read needs chunk " + std::to_string(c));
}

std::vector<ChunkRange>
Reader::region_chunk_ranges(uint32_t first, uint32_t count, const RegionArg* region) const
{
    return aqz::region_chunk_ranges(*ad_, first, count, region);
}

void
Reader::load_stats(uint64_t* decoded, uint64_t* copied)
{
    if (loaded_ == Loaded::None)
        throw Error(1, "no layer loaded");
    hip_check(hipEventSynchronize(load_ev_), "hipEventSynchronize");
    uint64_t sum = stat_decoded_;
    if (ranged_) {
        const dec::ByteRange* spans =
          reinterpret_cast<const dec::ByteRange*>(h_ranges_.p) + g_.n_chunks;
        sum = 0;
        for (uint32_t q = 0; q < g_.n_chunks; ++q)
            sum += spans[q].hi - spans[q].lo;
    }
    if (decoded)
        *decoded = sum;
    if (copied)
        *copied = stat_copied_;
}

std::vector<uint32_t>
Reader::region_chunks(uint32_t first, uint32_t count, const RegionArg* region) const
{
    return aqz::region_chunks(*ad_, first, count, region);
}

void
Reader::read_region(uint32_t first, uint32_t count, const RegionArg* region, void* dst,
                    uint64_t dst_row_stride, uint64_t dst_frame_stride, hipStream_t stream)
{
    if (loaded_ == Loaded::None)
        throw Error(1, "no layer loaded");
    if (!region)
        throw Error(1, "null region");
    if (count == 0 || uint64_t(first) + count > g_.n_frames)
        throw Error(1, "frame range empty or outside the layer");
    unsplit::RegionParams q{};
    if (!unsplit::make_region(g_, region->x0, region->y0, region->width, region->height,
                              dst_row_stride, q.r)) {
        unsplit::Region probe;
        if (!unsplit::make_region(g_, region->x0, region->y0, region->width, region->height,
                                  ~uint64_t(0), probe))
            throw Error(1, "region empty or outside the frame");
        throw Error(1, "dst_row_stride below the region's row bytes");
    }
    if (!dst)
        throw Error(1, "null destination");
    if (dst_frame_stride < unsplit::region_frame_extent(g_, q.r))
        throw Error(1, "dst_frame_stride below the region's frame extent");
    if (windowed_)
        check_window(first, count, q.r, *region);
    q.p.g = g_;
    q.p.src = src_;
    q.p.chunk_src = d_chunk_src_;
    q.p.tab_grp = d_tab_grp_;
    q.p.tab_off = d_tab_off_;
    q.p.dst = static_cast<uint8_t*>(dst);
    q.p.dst_stride = dst_frame_stride;
    q.p.first = first;
    q.p.count = count;
    // the load may have been enqueued on another stream
    hip_check(hipStreamWaitEvent(stream, load_ev_, 0), "hipStreamWaitEvent");
    const uint64_t align = src_align_ | uint64_t(reinterpret_cast<uintptr_t>(dst)) |
                           dst_row_stride | dst_frame_stride;
    hip_check(launch_unsplit_region(q, align, stream), "unsplit region launch");
    hip_check(hipEventRecord(read_ev_, stream), "hipEventRecord");
    read_pending_ = true;
}

void
Reader::status(uint32_t* status, size_t cap, uint32_t* n_bad)
{
    if (loaded_ == Loaded::None)
        throw Error(1, "no layer loaded");
    const uint32_t n = g_.n_chunks;
    if (status && cap < n)
        throw Error(2, "status array below chunks_per_layer");
    hip_check(hipEventSynchronize(load_ev_), "hipEventSynchronize");
    if (loaded_ == Loaded::Decoded) {
        std::fill(chunk_status_.begin(), chunk_status_.end(), uint32_t(dec::kSkipped));
        for (uint32_t q = 0; q < loaded_frames_; ++q)
            chunk_status_[h_order_[q]] = h_status_[q];
    } else if (loaded_ == Loaded::Chunks) {
        for (uint32_t c = 0; c < n; ++c)
            chunk_status_[c] = h_chunk_src_[c] == unsplit::kNoChunk ? dec::kSkipped : dec::kOk;
    }
    uint32_t bad = 0;
    for (uint32_t c = 0; c < n; ++c) {
        // a chunk outside the window of a region load was not looked at
        const uint32_t st = windowed_ && !window_[c] ? kNotLoaded : chunk_status_[c];
        if (status)
            status[c] = st;
        bad += st > dec::kSkipped && st != kNotLoaded;
    }
    if (n_bad)
        *n_bad = bad;
}

} // namespace aqz
