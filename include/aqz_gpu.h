/*
 * aqz_gpu.h -- C ABI of the MI355X-native multiscale-pyramid + chunk-tile
 * stage for acquire-zarr.
 *
 * Plain C, plain pointers and sizes.  Every call returns a status code with
 * the numeric values of ZarrStatusCode (reference include/zarr.types.h:13-31)
 * and never lets a C++ exception or a HIP error cross the boundary (a HIP
 * error maps to AQZ_STATUS_INTERNAL_ERROR and is sticky on the object, like
 * ZarrStream_s::error_, reference src/streaming/zarr.stream.cpp:1442-1449).
 *
 * Objects are not thread-safe: like the reference Downsampler / Array they
 * are driven from one consumer thread (reference zarr.stream.cpp:1683-1684).
 *
 * Which reference interface each entry point replaces is noted per function
 * (paths relative to /root/reference).
 */
#ifndef AQZ_GPU_H
#define AQZ_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (== ZarrStatusCode, include/zarr.types.h:13-31) ---- */
typedef int32_t aqz_status;
#define AQZ_STATUS_SUCCESS 0
#define AQZ_STATUS_INVALID_ARGUMENT 1
#define AQZ_STATUS_OVERFLOW 2
#define AQZ_STATUS_INVALID_INDEX 3
#define AQZ_STATUS_NOT_YET_IMPLEMENTED 4
#define AQZ_STATUS_INTERNAL_ERROR 5
#define AQZ_STATUS_OUT_OF_MEMORY 6
#define AQZ_STATUS_INVALID_SETTINGS 9
#define AQZ_STATUS_WRITE_OUT_OF_BOUNDS 12

/* ---- enums: numeric values of ZarrDataType (zarr.types.h:49-62),
 *      ZarrDimensionType (:81-88), ZarrDownsamplingMethod (:90-97) ------- */
enum
{
    AQZ_DTYPE_UINT8 = 0,
    AQZ_DTYPE_UINT16,
    AQZ_DTYPE_UINT32,
    AQZ_DTYPE_UINT64,
    AQZ_DTYPE_INT8,
    AQZ_DTYPE_INT16,
    AQZ_DTYPE_INT32,
    AQZ_DTYPE_INT64,
    AQZ_DTYPE_FLOAT32,
    AQZ_DTYPE_FLOAT64,
    AQZ_DTYPE_COUNT
};
enum
{
    AQZ_DIM_SPACE = 0,
    AQZ_DIM_CHANNEL,
    AQZ_DIM_TIME,
    AQZ_DIM_OTHER
};
enum
{
    AQZ_METHOD_DECIMATE = 0,
    AQZ_METHOD_MEAN,
    AQZ_METHOD_MIN,
    AQZ_METHOD_MAX,
    AQZ_METHOD_COUNT
};

/* where a frame pointer lives */
enum
{
    AQZ_MEM_HOST = 0,        /* pageable host memory (copied to pinned staging) */
    AQZ_MEM_DEVICE = 1,      /* already resident in this device's HBM */
    AQZ_MEM_HOST_PINNED = 2  /* page-locked host memory (e.g. aqz_host_alloc):
                                DMA'd straight to the device, asynchronously */
};

/* The pixel-geometry subset of ZarrDimensionProperties
 * (zarr.types.h:120-133): name/unit/scale do not affect the data path. */
typedef struct
{
    int32_t type;               /* AQZ_DIM_* */
    uint32_t array_size_px;     /* 0 = unbounded (append dimension only) */
    uint32_t chunk_size_px;
    uint32_t shard_size_chunks;
} aqz_dimension;

/* Mirrors the array part of ZarrArraySettings (zarr.types.h:157-169). */
typedef struct
{
    const aqz_dimension* dimensions; /* acquisition order, slowest first */
    size_t dimension_count;          /* >= 2; last two are Space (y, x) */
    int32_t data_type;               /* AQZ_DTYPE_* */
    int32_t multiscale;              /* bool */
    int32_t downsampling_method;     /* AQZ_METHOD_* */
    uint32_t max_levels;             /* 0 = no limit */
    const size_t* storage_dimension_order; /* NULL = acquisition order */
    int32_t device;                  /* HIP device ordinal */
} aqz_array_desc;

const char* aqz_version(void);
const char* aqz_status_message(aqz_status status);
/* The message of the last failed call on this thread ("" if none): what
 * the reference passes to LOG_ERROR before mapping an exception to a status
 * (src/streaming/zarr.stream.cpp:1704-1719, src/logger/logger.hh). */
const char* aqz_last_error(void);
/* Number of HIP devices visible (0 when no GPU). */
aqz_status aqz_device_count(int32_t* count);

/* ======================================================================
 * Host index math -- ArrayDimensions (src/streaming/array.dimensions.hh:45)
 * Pure host C++; usable without a GPU.
 * ==================================================================== */
typedef struct aqz_dims aqz_dims;

/* ArrayDimensions::ArrayDimensions (array.dimensions.cpp:137-189), including
 * the 2-D phantom-dimension prepend and storage_dimension_order. */
aqz_status aqz_dims_create(const aqz_dimension* dims, size_t ndims,
                           int32_t data_type, const size_t* storage_order,
                           aqz_dims** out);
void aqz_dims_destroy(aqz_dims* d);
size_t aqz_dims_ndims(const aqz_dims* d);
/* storage-order dimension i */
aqz_status aqz_dims_get(const aqz_dims* d, size_t i, aqz_dimension* out);
/* array.dimensions.cpp:264-282 */
uint32_t aqz_dims_tile_group_offset(const aqz_dims* d, uint64_t frame_id);
/* array.dimensions.cpp:284-314 */
uint64_t aqz_dims_chunk_internal_offset(const aqz_dims* d, uint64_t frame_id);
/* array.dimensions.cpp:232-262 */
uint32_t aqz_dims_chunk_lattice_index(const aqz_dims* d, uint64_t frame_id,
                                      uint32_t dim_index);
/* array.dimensions.cpp:602-620 */
uint64_t aqz_dims_transpose_frame_id(const aqz_dims* d, uint64_t frame_id);
uint64_t aqz_dims_bytes_per_chunk(const aqz_dims* d);
uint32_t aqz_dims_number_of_chunks_in_memory(const aqz_dims* d);
uint64_t aqz_dims_frames_per_chunk_layer(const aqz_dims* d);
/* array.dimensions.cpp:393-548 */
uint32_t aqz_dims_shard_index_for_chunk(const aqz_dims* d, uint32_t chunk);
uint32_t aqz_dims_shard_internal_index(const aqz_dims* d, uint32_t chunk);
/* chunks_per_shard, number_of_shards (one append-dimension shard row) and
 * chunk_layers_per_shard (array.dimensions.cpp:376-392); any may be NULL. */
aqz_status aqz_dims_shard_geometry(const aqz_dims* d, uint32_t* chunks_per_shard,
                                   uint32_t* n_shards, uint32_t* layers_per_shard);
/* skipped_internal_indices_for_shard_layer (array.dimensions.cpp:424-453):
 * the internal indices of `shard` that chunk layer `layer` (< layers per
 * shard) leaves unfilled -- ragged padding, skipped so the shard's
 * countdown completes.  Writes min(count, cap) of them to out (may be NULL
 * with cap 0) and the count to *n. */
aqz_status aqz_dims_skipped_internal_indices(const aqz_dims* d, uint32_t shard,
                                             uint32_t layer, uint32_t* out, size_t cap,
                                             size_t* n);
/* supports_dim1_banding, dim1_band_count, frames_per_dim1_band,
 * chunks_per_dim1_band (array.dimensions.cpp:344-373) */
aqz_status aqz_dims_dim1_banding(const aqz_dims* d, int32_t* supported,
                                 uint32_t* n_bands, uint64_t* frames_per_band,
                                 uint32_t* chunks_per_band);

/* Level geometry of the pyramid: Downsampler::make_writer_configurations_
 * (src/streaming/downsampler.cpp:494-597).  dims in storage order; writes the
 * number of levels (including level 0) and, if out_dims != NULL, the dims of
 * every level (n_levels * ndims entries, ndims after the 2-D prepend). */
aqz_status aqz_pyramid_levels(const aqz_dimension* dims, size_t ndims,
                              uint32_t max_levels, uint32_t* n_levels,
                              aqz_dimension* out_dims, size_t out_cap);

/* ======================================================================
 * Downsampler -- drop-in for zarr::Downsampler (src/streaming/downsampler.hh:
 * 12-64): same level geometry, same add/take contract, same cascade state
 * machine (downsampler.cpp:306-414), pixels computed on the GPU.
 * ==================================================================== */
typedef struct aqz_downsampler aqz_downsampler;

/* Downsampler::Downsampler(config, method) (downsampler.cpp:249-304).
 * Invalid dtype/method -> AQZ_STATUS_INVALID_ARGUMENT (the reference throws). */
aqz_status aqz_downsampler_create(const aqz_array_desc* desc,
                                  aqz_downsampler** out);
void aqz_downsampler_destroy(aqz_downsampler* ds);
/* writer_configurations().size() */
uint32_t aqz_downsampler_n_levels(const aqz_downsampler* ds);
/* writer_configurations().at(level)->dimensions (storage order) */
aqz_status aqz_downsampler_level_dims(const aqz_downsampler* ds,
                                      uint32_t level, aqz_dimension* out,
                                      size_t cap, size_t* ndims);
/* Downsampler::add_frame (downsampler.cpp:306-401).  frame is level-0 pixels,
 * nbytes >= width*height*bpp, mem = AQZ_MEM_HOST or AQZ_MEM_DEVICE. */
aqz_status aqz_downsampler_add_frame(aqz_downsampler* ds, const void* frame,
                                     size_t nbytes, int32_t mem);
/* Downsampler::take_frame (downsampler.cpp:403-414): *found = 0 if no frame
 * waits at `level`; otherwise copies it to dst (mem says where dst is). */
aqz_status aqz_downsampler_take_frame(aqz_downsampler* ds, uint32_t level,
                                      void* dst, size_t cap, int32_t mem,
                                      size_t* nbytes, int32_t* found);
/* Downsampler::downsampling_method (downsampler.cpp:422-438):
 * "decimate" | "local_mean" | "local_min" | "local_max" */
const char* aqz_downsampler_method_name(const aqz_downsampler* ds);
/* Downsampler::get_metadata (downsampler.cpp:440-485) as JSON text:
 * byte-identical to the reference's get_metadata().dump(), the block
 * MultiscaleArray embeds in zarr.json (multiscale.array.cpp:271).  With
 * buf == NULL only *len is set; cap must hold *len + 1 bytes. */
aqz_status aqz_downsampler_metadata_json(const aqz_downsampler* ds, char* buf,
                                         size_t cap, size_t* len);
/* The same two, from the method value alone (pure host, no GPU):
 * "" / AQZ_STATUS_INVALID_ARGUMENT for a method outside AQZ_METHOD_*. */
const char* aqz_downsampling_method_name(int32_t method);
aqz_status aqz_downsampling_metadata_json(int32_t method, char* buf, size_t cap,
                                          size_t* len);

/* ======================================================================
 * Stage -- the device-resident hot path of MultiscaleArray::write_frame
 * (src/streaming/multiscale.array.cpp:57-74, 291-325): level-0 tile split
 * (Array::write_frame_to_chunks_, array.cpp:507-622) + pyramid
 * (Downsampler::add_frame) + tile split of every level, written straight
 * into device-resident chunk layers with per-chunk has_data flags
 * (Chunk::write_tile_rows, chunk.cpp:17-58).
 *
 * A "chunk layer" of a level = number_of_chunks_in_memory chunks of
 * bytes_per_chunk bytes, chunk c at c*bytes_per_chunk (the reference's
 * Array::chunks_ vector, array.cpp:575-583), covering frames_per_chunk_layer
 * consecutive frames of that level.  The stage keeps `layer_slots` layers
 * per level resident in HBM as a ring.
 * ==================================================================== */
typedef struct aqz_stage aqz_stage;

typedef struct
{
    uint32_t layer_slots;      /* resident chunk layers per level (>=1; 0 = 2) */
    uint32_t max_batch_frames; /* frames per internal launch (0 = 64) */
    uint64_t first_frame;      /* level-0 frame id of this stage's first
                                  frame (z-slab sharding across GPUs: the
                                  slab's first plane); level k starts at
                                  first_frame * planes_k / planes_0, which
                                  must be exact.  0 = a whole stream. */
    uint32_t z_slab_begin;
    uint32_t z_slab_end;       /* z-slab schedule over a stream of volumes
                                  (BASELINE configs[3]): the stage
                                  receives only planes [begin, end) of every
                                  z stack (the level-0 dim ndims-3; a stack
                                  is one index of the dims before it), in
                                  order.  Frame ids skip the other planes:
                                  after each slab every level's frame id
                                  jumps by planes_k - (end_k - begin_k), so
                                  z pairs (Downsampler::add_frame's
                                  level_frame_count_ % planes,
                                  downsampler.cpp:358-389) and chunk
                                  placement (array.dimensions.cpp:264-314)
                                  stay those of the whole stream.  begin and
                                  end must scale exactly to every level
                                  (multiples of 2^(z-halving levels)); the
                                  first frame is first_frame + begin, with
                                  first_frame a multiple of the stack size.
                                  0, 0 = every plane. */
    uint32_t placement_tries;  /* n > 1: time the chunk-layer rings'
                                  placement on random frames at creation
                                  (aqz_stage_placement_report,
                                  aqz_gpu_bench.h).  Rings of >= 256 MiB in
                                  all are placed in one arena of 2 MiB
                                  virtual-memory pieces, where the fused
                                  kernels run in the fast band on most boxes
                                  (DESIGN.md section 3).  The arena is timed
                                  against the stage's algorithmic bytes at
                                  the rate of a streaming probe of the same
                                  memory; only when it is more than 3% over
                                  that, up to n - 1 fresh arenas follow, each
                                  made while the best is held and freed at
                                  once if slower.  The transient peak (one
                                  batch of random frames and a second ring
                                  set) is in aqz_stage_estimate_memory.
                                  0/1 = none. */
    uint32_t level0_split_on_host; /* 1: the device does not tile-split level
                                  0 (no level-0 ring in HBM); the caller
                                  splits level 0 on the host from the frames
                                  it holds (aqz_stage_split_level0_host /
                                  _rows): a raw hand-off
                                  then moves H2D 1x and D2H 1/3x of the input
                                  instead of D2H 4/3x.  Level-0 hand-off calls
                                  (copy_layer*, copy_band_async,
                                  compress_layer, device_layer,
                                  import_frames) return
                                  AQZ_STATUS_INVALID_ARGUMENT.  Not with an
                                  XY-transposed storage order
                                  (AQZ_STATUS_INVALID_SETTINGS). */
} aqz_stage_options;

typedef struct
{
    uint64_t bytes_per_chunk;
    uint32_t chunks_per_layer;
    uint32_t layer_slots;
    uint64_t frames_per_layer;
    uint64_t frame_bytes;      /* width*height*bpp of this level */
    uint32_t width, height;
    uint64_t chunk_pitch;      /* device bytes from chunk c to chunk c+1 of
                                  a resident layer (>= bytes_per_chunk; the
                                  pad staggers chunks over HBM channels).
                                  Host copies are packed at bytes_per_chunk. */
} aqz_level_layout;

aqz_status aqz_stage_create(const aqz_array_desc* desc,
                            const aqz_stage_options* opt, aqz_stage** out);
void aqz_stage_destroy(aqz_stage* st);
uint32_t aqz_stage_n_levels(const aqz_stage* st);
aqz_status aqz_stage_level_dims(const aqz_stage* st, uint32_t level,
                                aqz_dimension* out, size_t cap, size_t* ndims);
aqz_status aqz_stage_level_layout(const aqz_stage* st, uint32_t level,
                                  aqz_level_layout* out);
/* Run the stage on the HIP stream `stream` (a hipStream_t; NULL = the
 * stage's own stream).  All later work is enqueued there. */
aqz_status aqz_stage_set_stream(aqz_stage* st, void* stream);
/* Make the stage's stream wait for all work enqueued so far on `stream`
 * (a hipStream_t): append device frames produced there without a host
 * synchronisation (e.g. a torch stream that filled them). */
aqz_status aqz_stage_wait_stream(aqz_stage* st, void* stream);
/* Append n_frames full level-0 frames (contiguous, frame after frame; pitched
 * rows, sub-rectangles of a larger canvas and strided views go to
 * aqz_stage_append_strided, below, without a packing copy).
 * Equivalent to n_frames calls of MultiscaleArray::write_frame.
 *  - AQZ_MEM_HOST: copied into a pinned staging buffer by a few host threads
 *    before return, so the caller may reuse it at once, as with
 *    ZarrStream_append (frame.queue.cpp:37-39);
 *  - AQZ_MEM_HOST_PINNED (a camera's DMA ring) and AQZ_MEM_DEVICE: read
 *    asynchronously; keep the bytes unchanged until aqz_stage_frames_consumed
 *    counts them (or aqz_stage_synchronize returns).
 * The H2D runs on the stage's copy stream and overlaps earlier batches'
 * kernels and hand-off copies.
 * Source address (AQZ_MEM_DEVICE): any address aligned to the pixel size is
 * accepted and gives the same chunk layers.  A 16-byte-aligned address
 * whose rows are a multiple of 16 bytes (for an XY-swapped storage order:
 * the acquisition rows) takes the fast kernels; any other is read one pixel
 * at a time by the bounds-checked edge kernel (2-D), the generic one-level
 * cascade (2x2x2) or the separate transpose pass (XY), which are slower.
 * Host sources are staged into 16-byte-aligned device buffers. */
aqz_status aqz_stage_append(aqz_stage* st, const void* frames,
                            uint64_t n_frames, int32_t mem);
/* aqz_stage_append for pitched frames: `frames` points at pixel (0, 0) of the
 * first frame, and row y of frame k starts at frames + k * frame_stride +
 * y * row_stride (bytes).  Each row holds W * bpp bytes; W and H are those of
 * the frames as appended (for an XY-swapped storage order: the acquisition
 * rows).  Covers a frame grabber's line pitch, a sub-rectangle of a larger
 * sensor frame and a strided view of a tensor.
 * Contract: only bytes of pixels inside these rectangles are ever read.  The
 * bytes between rows may belong to someone else, and the last rectangle may
 * end at the end of an allocation.
 * The result is defined as the chunk layers and has_data flags that
 * aqz_stage_append gives for the same pixels packed contiguously.  Every
 * memory kind works; lifetime and aqz_stage_frames_consumed are those of
 * aqz_stage_append (a pinned source whose pitch the runtime's 2-D copy
 * refuses is staged like a pageable one and consumed on return); bounds
 * (status 12), z slabs, first_frame and batching too.  Strides of W * bpp and
 * W * H * bpp are exactly aqz_stage_append.
 * AQZ_STATUS_INVALID_ARGUMENT with an aqz_last_error text, nothing enqueued
 * and frames_written unchanged: row_stride < W * bpp; frame_stride <
 * (H - 1) * row_stride + W * bpp; either stride or the address no multiple of
 * the pixel size; n_frames * frame_stride overflowing 64 bits; a stage
 * created with level0_split_on_host (its host split takes contiguous host
 * frames).
 * Routes.  Host sources are packed on their way into the stage's contiguous
 * staging buffers (pageable: by the host threads' row copy; pinned: by a 2-D
 * DMA) and run no extra kernel.  A device source whose address, row_stride
 * and frame_stride are multiples of 16 is read in place by the fused kernels
 * (2-D stages; on a 2x2x2 stage the whole z groups of a batch that the pair
 * kernel takes) when the storage order is not XY-swapped.  Any other device
 * source -- a misaligned pitch, XY storage orders, the frames of a 2x2x2
 * batch that go to the generic cascade, non-default bench tuning -- is first
 * packed by a copy kernel into a stage-owned buffer of max_batch_frames
 * frames.  That buffer is allocated by the first packed append;
 * aqz_stage_memory_usage reports it from then on, and it is outside
 * aqz_stage_estimate_memory, like the verify decoder's state.
 * aqz_stage_source_report (aqz_gpu_bench.h) counts the frames by route. */
aqz_status aqz_stage_append_strided(aqz_stage* st, const void* frames, uint64_t n_frames,
                                    int32_t mem, uint64_t row_stride, uint64_t frame_stride);
aqz_status aqz_stage_synchronize(aqz_stage* st);
/* frames written so far to `level` (Array::frames_written_) */
uint64_t aqz_stage_frames_written(const aqz_stage* st, uint32_t level);
/* Level-0 frames appended so far whose source bytes the stage has finished
 * reading (in append order): their source buffers may be reused. */
uint64_t aqz_stage_frames_consumed(aqz_stage* st);
/* Block (on events, no spin) until at least `frames` appended level-0
 * frames have been read: the reference's frame queue hands its buffer back
 * when the consumer pops it (frame.queue.cpp:48-73); a caller that appends
 * pinned batches from a double buffer waits here before refilling one. */
aqz_status aqz_stage_wait_consumed(aqz_stage* st, uint64_t frames);
/* Copy chunk layer `layer` of `level` (must still be resident) to dst
 * (bytes_per_chunk*chunks_per_layer bytes) and its has_data flags (one byte
 * per chunk, 1 = some byte of the chunk is nonzero).  Synchronizes.  Frames
 * of a layer not yet written read as unspecified bytes until the layer is
 * complete or aqz_stage_finalize ran.  mem = where dst lives. */
aqz_status aqz_stage_copy_layer(aqz_stage* st, uint32_t level, uint64_t layer,
                                void* dst, size_t cap, uint8_t* has_data,
                                size_t has_data_cap, int32_t mem);
/* Asynchronous hand-off of a resident chunk layer (outputs D2H
 * straight into host chunk buffers): enqueues, after all work appended so
 * far, a D2H copy of the layer into dst (pinned memory for a real overlap;
 * cap >= bytes_per_chunk * chunks_per_layer) and of its has_data bytes into
 * has_data (NULL to skip), on the stage's hand-off stream.  Returns at once;
 * the ring slot is not rewritten until the copy has finished.  The copies
 * are complete after aqz_stage_wait_copies or aqz_stage_synchronize. */
aqz_status aqz_stage_copy_layer_async(aqz_stage* st, uint32_t level,
                                      uint64_t layer, void* dst, size_t cap,
                                      uint8_t* has_data, size_t has_data_cap);
aqz_status aqz_stage_wait_copies(aqz_stage* st);
/* Hand-off tickets.  Every aqz_stage_copy_layer_async,
 * aqz_stage_copy_band_async and aqz_stage_copy_compressed_async call that
 * succeeds is one ticket, numbered 1, 2, ... in call order;
 * aqz_stage_last_ticket returns the newest.  aqz_stage_copies_completed
 * returns (without blocking) how many tickets have completed -- their
 * destination bytes are in place -- and tickets complete in order.
 * aqz_stage_wait_ticket blocks until ticket `ticket` has completed.  With
 * these a caller installs each handed-off unit into its host chunk buffers
 * (Array::chunks_) when its copy lands, in frame order, and never waits
 * for copies issued after it (cf. the flush in array.cpp:209-219). */
uint64_t aqz_stage_last_ticket(const aqz_stage* st);
uint64_t aqz_stage_copies_completed(aqz_stage* st);
aqz_status aqz_stage_wait_ticket(aqz_stage* st, uint64_t ticket);

/* ---- dim-1 banding ---------------------------------------------------------
 * Array::flush_completed_bands_ (array.cpp:873-908) flushes the chunks of a
 * band of dimension 1 as soon as its frames are written, before the whole
 * chunk layer is: ArrayDimensions::supports_dim1_banding, dim1_band_count,
 * frames_per_dim1_band, chunks_per_dim1_band (array.dimensions.cpp:344-373).
 * Band b of a layer is the contiguous chunk range
 * [b * chunks_per_band, (b + 1) * chunks_per_band). */
aqz_status aqz_stage_band_geometry(const aqz_stage* st, uint32_t level,
                                   int32_t* supported, uint32_t* n_bands,
                                   uint64_t* frames_per_band,
                                   uint32_t* chunks_per_band);
/* Asynchronous hand-off of one complete band of a resident layer, like
 * aqz_stage_copy_layer_async for its chunk range: dst receives
 * chunks_per_band * bytes_per_chunk bytes, has_data (NULL to skip)
 * chunks_per_band flags.  The band must be complete: all its frames
 * written (frames_written(level) >= layer * frames_per_layer +
 * (band + 1) * frames_per_band), or the layer finalized. */
aqz_status aqz_stage_copy_band_async(aqz_stage* st, uint32_t level,
                                     uint64_t layer, uint32_t band, void* dst,
                                     size_t cap, uint8_t* has_data,
                                     size_t has_data_cap);

/* ---- memory accounting ------------------------------------------------------
 * What the stage holds, for ZarrStream_get_current_memory_usage
 * (zarr.stream.cpp:1057-1068) and ZarrStreamSettings_estimate_max_memory_usage
 * (acquire.zarr.cpp:216-314) to include. */
typedef struct
{
    uint64_t device_bytes; /* HBM: chunk-layer rings, has_data words, frame
                              tables, scratch, H2D staging, compressed frames */
    uint64_t pinned_bytes; /* page-locked host memory: host-source staging,
                              compressed-offset read-back */
} aqz_memory_usage;
/* Bytes currently allocated by the stage. */
aqz_status aqz_stage_memory_usage(const aqz_stage* st, aqz_memory_usage* out);
/* Upper bound of what a stage created with (desc, opt) allocates, compressed
 * hand-off excluded (add aqz_compressor_max_bytes per compressed slot and
 * aqz_compressor_scratch_bytes per compressed level).  No GPU needed. */
aqz_status aqz_stage_estimate_memory(const aqz_array_desc* desc,
                                     const aqz_stage_options* opt,
                                     aqz_memory_usage* out);
/* Pin the calling thread to the CPUs of the NUMA node of the stage's device
 * (the CPUs the stage's own host threads run on; no-op when unknown): for a
 * caller's threads that feed the stage or read its hand-off buffers.  The
 * reference pins none of its threads (thread.pool.cpp:6-20). */
aqz_status aqz_stage_bind_host_thread(const aqz_stage* st);
/* Page-locked host memory for frames and hand-off buffers. */
aqz_status aqz_host_alloc(size_t bytes, void** out);
void aqz_host_free(void* p);
/* Device pointers of a resident layer (for device-side consumers).  Chunk c
 * starts at chunks + c * chunk_pitch (aqz_level_layout).  Chunk c has data iff has_data[c] == layer / layer_slots + 1 (the words carry the
 * ring-slot generation, so they are never cleared). */
aqz_status aqz_stage_device_layer(aqz_stage* st, uint32_t level,
                                  uint64_t layer, void** chunks,
                                  uint32_t** has_data);
/* ---- chunk compression on the device ----------------
 * ZarrCompressionSettings (zarr.types.h:112-122) as applied by
 * Chunk::compress_and_take_buffer (chunk.cpp:78-106) ->
 * zarr::compress_in_place (zarr.common.cpp:106-140) -> blosc_compress_ctx.
 * codec: ZarrCompressionCodec values.
 *  - AQZ_CODEC_BLOSC_LZ4: blosc1 frames made on the device (shuffle +
 *    LZ4); clevel 0 stores every chunk as a memcpyed frame, levels 1-9 run
 *    the same GPU match finder.
 *  - AQZ_CODEC_BLOSC_ZSTD: blosc1 frames made on the device: every block
 *    (256 KiB) shuffled, then one zstd frame per block (zarr.common.cpp:
 *    106-140 with "zstd"); blosc clevel 0 stores memcpyed frames.
 *  - AQZ_CODEC_ZSTD: one zstd frame per chunk (ZSTD_compress,
 *    zarr.common.cpp:142-166), made on the device.
 *  The device zstd encoder: Huffman literals (one table per 64 KiB group of
 *  a shuffled block -- per bit plane under bitshuffle at clevel >= 7 -- or
 *  per 256 KiB of unshuffled data), sequence tables fitted per
 *  frame, a greedy LZ parse in 4 KiB units; the level sets how far back
 *  matches reach (zstd level L; blosc clevel c is L = 2c - 1): plain zstd
 *  L 1-2 unit-local, L 3-6 + far candidates from a 2^17-entry table over
 *  the whole chunk, L >= 7 a 2^18-entry table; blosc-zstd with bitshuffle
 *  L >= 3 a 2^15-entry table per block.  Ratios on camera-like and dim u16
 *  data are within ~1% (blosc-zstd) and ~7% (plain zstd L 5) of libzstd
 *  (c-blosc clevel 5 / ZSTD_compress level 5).  With
 *  AQZ_ZSTD_HOST=1 in the environment the zstd codecs run on a host pool
 *  instead (device shuffle, D2H, the system's libzstd.so.1 at the clevel ->
 *  zstd level map of c-blosc; absent library ->
 *  AQZ_STATUS_NOT_YET_IMPLEMENTED), byte for byte what libzstd makes.
 *  Frames decode (any blosc1 / zstd decoder) to the chunk bytes exactly;
 *  their compressed bytes differ from c-blosc's and libzstd's (block size,
 *  match finder, no stream split for blosc-zstd). */
#define AQZ_CODEC_NONE 0
#define AQZ_CODEC_BLOSC_LZ4 1
#define AQZ_CODEC_BLOSC_ZSTD 2
#define AQZ_CODEC_ZSTD 3
typedef struct
{
    int32_t codec;   /* ZarrCompressionCodec */
    int32_t clevel;  /* 0-9 */
    int32_t shuffle; /* 0 none, 1 byte (BLOSC_SHUFFLE), 2 bit (BLOSC_BITSHUFFLE) */
} aqz_compression;

/* Compress resident layer `layer` of `level` into blosc1 frames, one per
 * chunk with data (chunks without data are skipped, like the reference's
 * skip_chunk), back to back in SHARD-MAJOR order: the chunks of shard 0 by
 * shard_internal_index, then shard 1, ... (aqz_stage_compressed_entries
 * lists them), so each shard's frames of the layer are one contiguous run
 * that Shard::write_chunk would append at the shard's file offset.  Runs on the hand-off stream
 * after the kernels that wrote the layer; the slot is not reused until it
 * has been read. */
aqz_status aqz_stage_compress_layer(aqz_stage* st, uint32_t level, uint64_t layer,
                                    const aqz_compression* comp);
/* Waits for that compression.  offsets[i] = start of the i-th frame in
 * output order, offsets[i+1] - offsets[i] its size (0: skipped),
 * offsets[chunks_per_layer] = total bytes.  n >= chunks_per_layer + 1. */
aqz_status aqz_stage_compressed_offsets(aqz_stage* st, uint32_t level,
                                        uint64_t layer, uint64_t* offsets, size_t n);
/* Copy of the layer's frames (total bytes) to dst: host or device,
 * asynchronous, complete after aqz_stage_wait_copies.  With AQZ_ZSTD_HOST=1
 * (zstd frames made on the host) dst is host memory, filled before the
 * call returns. */
aqz_status aqz_stage_copy_compressed_async(aqz_stage* st, uint32_t level,
                                           uint64_t layer, void* dst, size_t cap);
/* *done = 1 once the compression of that layer has finished (no wait): then
 * aqz_stage_compressed_offsets / _entries and aqz_stage_copy_compressed_async
 * do not block the caller.  A consumer thread issues the frames' D2H only
 * for finished layers, as the reference's flush jobs hand a chunk to its
 * shard once compress_and_take_buffer returned (array.cpp:722-736). */
aqz_status aqz_stage_compression_done(aqz_stage* st, uint32_t level, uint64_t layer,
                                      int32_t* done);

/* ---- shard packing -----------------------------------
 * The frames of a compressed layer in output order, with their place in
 * the shards (ArrayDimensions::shard_index_for_chunk / shard_internal_index,
 * array.dimensions.cpp:396-548; the internal index includes the layer's
 * position along the append dimension inside its shard). */
typedef struct
{
    uint32_t chunk;    /* chunk index inside the layer (Array::chunks_ slot) */
    uint32_t shard;    /* shard of the current append-dimension shard row */
    uint32_t internal; /* shard_internal_index */
    uint32_t reserved;
    uint64_t offset;   /* frame start inside the compressed layer */
    uint64_t nbytes;   /* frame bytes; 0 = no data (Shard::skip_chunk) */
} aqz_chunk_entry;
aqz_status aqz_stage_compressed_entries(aqz_stage* st, uint32_t level,
                                        uint64_t layer, aqz_chunk_entry* out,
                                        size_t n);
/* chunks_per_shard, number_of_shards (one append-dimension shard row) and
 * chunk layers per shard (array.dimensions.cpp:376-397) of a level. */
aqz_status aqz_stage_shard_geometry(const aqz_stage* st, uint32_t level,
                                    uint32_t* chunks_per_shard,
                                    uint32_t* number_of_shards,
                                    uint32_t* layers_per_shard);
/* Shard::write_table_ (shard.cpp:145-166): chunks_per_shard (offset,
 * extent) little-endian uint64 pairs -- UINT64_MAX for both when a chunk
 * was never written -- followed by the CRC-32C of those bytes; out holds
 * aqz_shard_table_bytes(chunks_per_shard) bytes.  The table goes at the end
 * of the shard (index_location "end"). */
size_t aqz_shard_table_bytes(uint32_t chunks_per_shard);
aqz_status aqz_shard_table(const uint64_t* offsets, const uint64_t* extents,
                           uint32_t chunks_per_shard, void* out, size_t cap);
uint32_t aqz_crc32c(const void* data, size_t n);

/* Stand-alone compressor (any AQZ_CODEC_*) for device-resident chunk arrays: chunk i of
 * n_chunks at chunks + i * pitch, chunk_bytes each; frames back to back at
 * dst (device, >= aqz_compressor_max_bytes), offsets (device, n_chunks + 1
 * uint64) as above.  Enqueued on `stream` (hipStream_t; NULL = default).
 * The frames of a run may add up to any size (the offsets are summed in 64
 * bits: five incompressible 1 GiB chunks pass 4 GiB).  One limit on the chunk
 * count: AQZ_CODEC_BLOSC_ZSTD with a shuffle that moves bytes (bit shuffle, or
 * byte shuffle of a typesize above 1) at clevel >= 1 takes at most 65535 chunks
 * per run; more is AQZ_STATUS_INVALID_ARGUMENT before anything is enqueued
 * (the same for a stage layer of that many chunks). */
typedef struct aqz_compressor aqz_compressor;
aqz_status aqz_compressor_create(uint64_t chunk_bytes, uint32_t typesize,
                                 const aqz_compression* comp, aqz_compressor** out);
void aqz_compressor_destroy(aqz_compressor* c);
uint64_t aqz_compressor_max_bytes(uint64_t chunk_bytes, uint32_t n_chunks);
/* Device scratch one compressor (or one level of a stage compressing its
 * layers) allocates to compress n_chunks chunks of chunk_bytes with `comp`
 * (an upper bound; the zstd codecs keep parse units, sequences and per-block
 * state at about 4x the layer).  0 on invalid settings.  No GPU needed. */
uint64_t aqz_compressor_scratch_bytes(const aqz_compression* comp, uint64_t chunk_bytes,
                                      uint32_t typesize, uint32_t n_chunks);
aqz_status aqz_compressor_run(aqz_compressor* c, const void* chunks, uint64_t pitch,
                              uint32_t n_chunks, void* dst, size_t dst_cap,
                              uint64_t* offsets, void* stream);
/* The blosc block size of the frames (recorded in each frame header; 0 for
 * plain zstd). */
uint32_t aqz_compressor_blocksize(const aqz_compressor* c);

/* z-slab assembly of one chunk layer (a volume stream sharded
 * over GPUs by z slabs, aqz_stage_options.z_slab_*): copy the tiles of
 * frames [first, first + count) of `layer` of `level` (frame ids inside the
 * layer) from stage src's resident layer into dst's, with their has_data
 * flags -- over xGMI when the stages' devices differ (peer access is
 * enabled on first use), on dst's stream after all work enqueued so far on
 * src's.  src = NULL zero-fills those frames in dst.  The two stages must
 * have the same array description and options apart from the device and
 * the slab.  The layer becomes resident in dst if it was not; src's ring
 * slot is not rewritten until the copy has read it.  dst then holds the
 * whole layer and hands it off (aqz_stage_copy_*_async,
 * aqz_stage_compress_layer) as if it had written every frame -- the chunk
 * buffers Array::write_frame_to_chunks_ fills (array.cpp:507-622). */
aqz_status aqz_stage_import_frames(aqz_stage* dst, aqz_stage* src, uint32_t level,
                                   uint64_t layer, uint32_t first, uint32_t count);

/* ---- level-0 tile split on the host (aqz_stage_options.
 * level0_split_on_host) ---------------------------------------------------
 * Array::write_frame_to_chunks_ (array.cpp:537-619) with
 * Chunk::write_tile_rows (chunk.cpp:17-58), run by the host on frames it
 * holds: tile t of level-0 frame f goes to chunk t + tile_group_offset(f)
 * of f's chunk layer, its rows at chunk_internal_offset(f) +
 * r * tile_cols * bpp (f transposed to storage order first,
 * array.cpp:557-566); ragged padding is not written; has_data[c] becomes 1
 * once a copied byte of chunk c is nonzero and is never cleared (zero it
 * when a layer starts).  dst holds the packed chunks [chunk0, chunk0 +
 * cap / bytes_per_chunk) of one layer -- the whole layer (chunk0 0), or a
 * dim-1 band (chunk0 = band * chunks_per_band) -- laid out as
 * aqz_stage_copy_layer_async / _band_async would write them; has_data has
 * has_data_cap >= that many bytes.  Every tile of every frame must fall in
 * that range (else AQZ_STATUS_INVALID_ARGUMENT).  Pure host work: no GPU
 * call, any thread. */
/* Frames [first_frame, first_frame + n_frames) (level-0 frame ids, in
 * acquisition order, frame after frame at `frames`; all in one chunk layer,
 * else AQZ_STATUS_INVALID_ARGUMENT), split by the stage's host threads (on
 * the NUMA node of its device). */
aqz_status aqz_stage_split_level0_host(aqz_stage* st, const void* frames, uint64_t n_frames,
                                       uint64_t first_frame, uint32_t chunk0, void* dst,
                                       size_t cap, uint8_t* has_data, size_t has_data_cap);
/* Rows [row_begin, row_end) of one level-0 frame, on the calling thread;
 * several threads may split disjoint rows of one frame at once.  frame_copy
 * (NULL: none): the same rows are also copied to this frame-sized buffer in
 * the same pass -- the hand-off's copy into its pinned batch
 * (ZarrStream_append's one copy, frame.queue.cpp:37-39). */
aqz_status aqz_stage_split_level0_rows(const aqz_stage* st, const void* frame,
                                       uint64_t frame_id, uint32_t row_begin,
                                       uint32_t row_end, void* frame_copy, uint32_t chunk0,
                                       void* dst, size_t cap, uint8_t* has_data,
                                       size_t has_data_cap);
/* The same split over an aqz_dims (the array's acquisition dims with its
 * storage order), no stage and no GPU. */
aqz_status aqz_dims_split_frame_rows(const aqz_dims* d, const void* frame, uint64_t frame_id,
                                     uint32_t row_begin, uint32_t row_end, uint32_t chunk0,
                                     void* dst, size_t cap, uint8_t* has_data,
                                     size_t has_data_cap);

/* Zero the not-yet-written frames of every level's last partial layer so
 * it can be flushed (the reference's lazily zeroed chunks, chunk.cpp:8-15).
 * The unpaired trailing z plane is dropped, as in the reference. */
aqz_status aqz_stage_finalize(aqz_stage* st);

/* ---- chunk decompression on the device ------------------------------------
 * The inverse of AQZ_CODEC_BLOSC_LZ4: blosc1 frames with the LZ4 codec, and
 * memcpyed frames, decoded where they lie in HBM.  The format contract is the
 * codec metadata the reference writes (array.cpp:340-360: "blosc", cname
 * "lz4", clevel, shuffle, typesize, blocksize 0): any conforming blosc1 v2
 * frame is accepted -- this library's (4 KiB streams) or c-blosc's own (any
 * block size, split or "don't split", byte shuffle, bitshuffle or none,
 * streams stored raw).  The reference has no read path; what a reader of its
 * output would run per chunk is blosc_decompress_ctx.
 * A malformed frame is a per-chunk status, never a fault: reads end at the
 * frame's end, writes at the chunk's end, and the other frames of the run
 * are decoded as if it were not there.
 *
 * The zstd codecs (AQZ_CODEC_BLOSC_ZSTD, AQZ_CODEC_ZSTD) are opt-in, because
 * their decoder needs device scratch the LZ4 one does not: a decoder made by
 * aqz_decompressor_create_for with AQZ_DECODE_CODEC_ZSTD also decodes blosc1
 * frames whose compressor code is zstd (each stream one zstd frame; memcpyed
 * frames included) and plain zstd frames that decode to exactly chunk_bytes
 * -- any conforming RFC 8878 frame without a dictionary (this library's and
 * libzstd's at any level: Single_Segment or windowed, any Frame_Content_Size
 * width, Raw / RLE / Compressed blocks, all literal kinds and table modes,
 * repeat offsets, matches across blocks at any distance).  A content checksum
 * is accounted for (its 4 bytes) and NOT verified.  A frame's kind comes from
 * its own first bytes, so one run may mix all of them. */
#define AQZ_DECODE_OK 0          /* the chunk holds the decoded bytes */
#define AQZ_DECODE_SKIPPED 1     /* zero-length frame: the chunk was zero-filled (an
                                    unwritten chunk reads as fill_value 0, array.cpp:279) */
#define AQZ_DECODE_BAD_HEADER 2  /* version, typesize 0, nbytes != chunk_bytes, cbytes !=
                                    frame size, blocksize 0 or no multiple of typesize, a
                                    block start outside the frame, or offsets that do not
                                    describe a frame inside frames_bytes */
#define AQZ_DECODE_CORRUPT 3     /* a stream record or an LZ4 sequence leaves its bounds; in
                                    a zstd frame, anything wrong inside the blocks (sizes,
                                    Huffman / FSE descriptions, bitstreams, sequences,
                                    offsets, output length) or after the last one */
#define AQZ_DECODE_UNSUPPORTED 4 /* a codec the decoder was not created for (blosc-zstd and
                                    plain zstd frames unless AQZ_DECODE_CODEC_ZSTD, blosc-lz4
                                    frames unless AQZ_DECODE_CODEC_LZ4); always: other blosc
                                    codecs, a zstd Dictionary_ID other than 0, a skippable
                                    zstd frame.  (For zstd frames BAD_HEADER covers: a
                                    stream or plain frame without the zstd magic, a reserved
                                    frame-header bit, a Frame_Content_Size that differs from
                                    the expected length, a header that does not fit.) */
#define AQZ_DECODE_CODEC_LZ4 1u  /* blosc1 frames with the LZ4 codec, memcpyed frames */
#define AQZ_DECODE_CODEC_ZSTD 2u /* blosc1 frames with the zstd codec, plain zstd frames */
/* Option bit of a codecs mask, valid only as AQZ_DECODE_CODEC_ZSTD | AQZ_DECODE_ZSTD_PARALLEL
 * (alone, or in a mask that also lists AQZ_DECODE_CODEC_LZ4, it is
 * AQZ_STATUS_INVALID_ARGUMENT and 0 bytes: a decoder with the option serves the zstd family
 * only, and LZ4 frames of its runs are AQZ_DECODE_UNSUPPORTED): plain zstd frames are decoded by block-parallel
 * kernels (entropy decode of all blocks at once, literal copies out of the match chain)
 * instead of one wave walking the frame.  The same frames are accepted, with the same
 * statuses and the same bytes; blosc1-zstd frames, and a plain frame with more than
 * max_chunk_bytes / 1024 + 16 blocks, are decoded by the serial kernel in the same run.
 * It costs the scratch aqz_decompressor_scratch_bytes_for describes. */
#define AQZ_DECODE_ZSTD_PARALLEL 4u
typedef struct aqz_decompressor aqz_decompressor;
/* A decoder with device scratch for runs of up to max_chunks frames of up to
 * max_chunk_bytes each (aqz_decompressor_scratch_bytes).  It decodes
 * AQZ_DECODE_CODEC_LZ4 only. */
aqz_status aqz_decompressor_create(uint64_t max_chunk_bytes, uint32_t max_chunks,
                                   aqz_decompressor** out);
/* The same for the codecs listed (AQZ_DECODE_CODEC_* or-ed, or
 * AQZ_DECODE_CODEC_ZSTD | AQZ_DECODE_ZSTD_PARALLEL; no codec or unknown bits:
 * AQZ_STATUS_INVALID_ARGUMENT).  Zero-length frames are skipped chunks whatever
 * the codecs. */
aqz_status aqz_decompressor_create_for(uint64_t max_chunk_bytes, uint32_t max_chunks,
                                       uint32_t codecs, aqz_decompressor** out);
void aqz_decompressor_destroy(aqz_decompressor* d);
/* Device bytes aqz_decompressor_create allocates: one slot per chunk, used by
 * frames whose blocks exceed the on-chip budget (32 KiB; c-blosc's frames of
 * large chunks).  0 on invalid sizes.  No GPU needed. */
uint64_t aqz_decompressor_scratch_bytes(uint64_t max_chunk_bytes, uint32_t max_chunks);
/* Device bytes aqz_decompressor_create_for allocates, exactly.  With
 * AQZ_DECODE_CODEC_ZSTD: the slot per chunk (max_chunk_bytes rounded up to 16;
 * shuffled blosc blocks and everything in compare mode are decoded there,
 * since zstd matches reach back farther than any on-chip window) plus the
 * Huffman-literal slots: min(max_chunk_bytes, 128 KiB) rounded up to 16, times
 * min(8, ceil(max_chunk_bytes / 32 KiB)) concurrent block decodes per chunk.
 * AQZ_DECODE_ZSTD_PARALLEL adds, with n = max_chunk_bytes and r16 = "rounded
 * up to 16":
 *   max_chunks * (64 * (n / 1024 + 16)     the block table, 64 bytes a block
 *                 + r16(n)                 Huffman literals of all blocks
 *                 + r16(12 * (n / 3)))     12-byte sequence records; a sequence
 *                                          regenerates at least 3 bytes
 *   + r16(8 * max_chunks) + 16             two words per frame, the count words
 * (divisions round down).  Nothing is allocated by aqz_decompressor_run.  0 on invalid arguments.  No
 * GPU needed. */
uint64_t aqz_decompressor_scratch_bytes_for(uint64_t max_chunk_bytes, uint32_t max_chunks,
                                            uint32_t codecs);
/* Decode n_chunks frames lying back to back at frames (device, frames_bytes
 * in all): frame i is bytes [offsets[i], offsets[i + 1]) -- offsets (device,
 * n_chunks + 1 uint64) as aqz_compressor_run and aqz_stage_compress_layer
 * write them; a zero-length frame is a skipped chunk.  Chunk i goes to
 * dst + i * pitch (device; chunk_bytes each, pitch >= chunk_bytes; the bytes
 * between chunks are not touched) and its AQZ_DECODE_* status to status[i]
 * (device).  Typesize and shuffle come from each frame's header.  Enqueued
 * on `stream` (hipStream_t; NULL = default); returns at once.  The contents
 * of a chunk whose status is an error are unspecified. */
aqz_status aqz_decompressor_run(aqz_decompressor* d, const void* frames, size_t frames_bytes,
                                const uint64_t* offsets, uint32_t n_chunks, void* dst,
                                uint64_t pitch, uint64_t chunk_bytes, uint32_t* status,
                                void* stream);

/* Decode the frames of compressed layer `layer` of `level` on the device and compare them
 * with the resident chunk layer.  frames == NULL: the stage's own compressed buffer.
 * Otherwise frames is a device copy in the same output order and with the same offsets
 * (e.g. after a round trip through the sink).  Enqueued on the hand-off stream after the
 * compression (the stream aqz_stage_compress_layer runs on).  The slot is not reused until
 * the comparison has read it.  The layer must have been compressed with AQZ_CODEC_BLOSC_LZ4
 * (any clevel) and still be resident (else AQZ_STATUS_INVALID_ARGUMENT); layers compressed
 * with a zstd codec return AQZ_STATUS_NOT_YET_IMPLEMENTED unless
 * aqz_stage_verify_prepare was called with AQZ_DECODE_CODEC_ZSTD.  A zstd layer whose
 * frames were made on the host (AQZ_ZSTD_HOST=1) has no device frames of its own: it is
 * refused with AQZ_STATUS_INVALID_ARGUMENT unless `frames` is given.  The first LZ4 verify
 * of a stage allocates the LZ4 decoder state (two words per chunk and slot, device and
 * pinned; no copy of the layer: the comparison happens as the blocks are un-shuffled),
 * which aqz_stage_memory_usage reports from then on. */
aqz_status aqz_stage_verify_layer(aqz_stage* st, uint32_t level, uint64_t layer,
                                  const void* frames, size_t frames_bytes);
/* Allocate now, for every level the stage splits on the device, the decoder state
 * aqz_stage_verify_layer needs for layers of the listed codecs (AQZ_DECODE_CODEC_* or-ed,
 * or AQZ_DECODE_CODEC_ZSTD | AQZ_DECODE_ZSTD_PARALLEL, which the zstd decoder is then created with;
 * no codec or unknown bits: AQZ_STATUS_INVALID_ARGUMENT); aqz_stage_memory_usage reports it from
 * this call on.  With AQZ_DECODE_CODEC_ZSTD that is, per level: the two words per chunk
 * and slot (device and pinned), and one zstd decoder for a layer slot's chunks
 * (aqz_decompressor_scratch_bytes_for(chunk bytes, chunks per layer,
 * AQZ_DECODE_CODEC_ZSTD)) -- one decoded copy of a layer slot's chunks, which the
 * comparison reads (zstd matches reach back up to the whole frame, so the compare cannot
 * happen as the blocks are un-shuffled, as it does for LZ4), plus the Huffman-literal
 * slots.  One decoder serves all slots of a level: verifies of a level run in order on
 * the hand-off stream.  Without this call nothing changes: zstd layers stay
 * AQZ_STATUS_NOT_YET_IMPLEMENTED and the first LZ4 verify allocates what it always did.
 * Calling it again adds the codecs not yet prepared; a zstd decoder prepared with the
 * other setting of AQZ_DECODE_ZSTD_PARALLEL is replaced. */
aqz_status aqz_stage_verify_prepare(aqz_stage* st, uint32_t codecs);
/* Waits.  *n_bad = chunks whose decoded bytes differ from the resident chunk or whose
 * decode status is an error.  A skipped chunk is good iff the resident chunk is all zero.
 * *first_bad = lowest such chunk index (aqz_chunk_entry.chunk), UINT32_MAX if none. */
aqz_status aqz_stage_verify_result(aqz_stage* st, uint32_t level, uint64_t layer,
                                   uint32_t* n_bad, uint32_t* first_bad);

/* ---- device reader: chunk layers and shards back to frames ------------------
 * The reference has no read path; these are the inverses of its write path.
 *
 * Inverse of aqz_shard_table (Shard::write_table_, shard.cpp:145-166); host
 * only.  table: the nbytes == aqz_shard_table_bytes(chunks_per_shard) bytes at
 * the end of a shard (else AQZ_STATUS_INVALID_ARGUMENT).  offsets / extents
 * (chunks_per_shard each; either may be NULL) get the little-endian pairs,
 * UINT64_MAX pairs for chunks never written; *crc_ok (may be NULL) = the
 * stored CRC-32C matches the table bytes.  A table whose CRC does not match is
 * still parsed. */
aqz_status aqz_shard_table_parse(const void* table, size_t nbytes, uint32_t chunks_per_shard,
                                 uint64_t* offsets, uint64_t* extents, int32_t* crc_ok);

/* A reader serves one array, i.e. one level: it turns a chunk layer of that
 * level -- raw, compressed with any AQZ_CODEC_*, or gathered from shard files
 * -- into row-major frames in device memory, in the order and orientation
 * the frames were appended (the inverse of Array::write_frame_to_chunks_,
 * array.cpp:537-619, of transpose_frame_id and of transpose_frame,
 * array.cpp:488-534).  Chunks never written read as zeros (fill_value 0,
 * array.cpp:279).  Levels >= 1 are stored in storage order throughout: a
 * reader for one takes that level's dims (aqz_stage_level_dims) and no
 * storage order. */
typedef struct aqz_reader aqz_reader;
typedef struct
{
    const aqz_dimension* dimensions; /* of this level, acquisition order */
    size_t dimension_count;
    int32_t data_type;               /* AQZ_DTYPE_* */
    const size_t* storage_dimension_order; /* level 0 only; NULL = acquisition order */
    uint32_t codecs;           /* AQZ_DECODE_CODEC_* or-ed, or AQZ_DECODE_CODEC_ZSTD |
                                  AQZ_DECODE_ZSTD_PARALLEL;
                                  0 = raw chunks only */
    uint64_t max_frames_bytes; /* device staging for frames given in host memory;
                                  0 = aqz_compressor_max_bytes(bytes_per_chunk,
                                  chunks_per_layer) */
    int32_t device;
} aqz_reader_desc;
/* Everything the reader will ever use is allocated here: the per-frame
 * tables, the chunk table, a decoded-layer buffer (chunks at bytes_per_chunk
 * rounded up to 16; only with codecs != 0), the staging buffer and the
 * decoder's scratch (aqz_decompressor_scratch_bytes_for).  Loading and
 * reading allocate no device memory. */
aqz_status aqz_reader_create(const aqz_reader_desc* desc, aqz_reader** out);
void aqz_reader_destroy(aqz_reader* r);
/* Device bytes aqz_reader_create allocates for desc, exactly.  0 for an
 * invalid description.  No GPU needed. */
uint64_t aqz_reader_device_bytes(const aqz_reader_desc* desc);
/* frame_bytes, frames_per_layer, chunks_per_layer, bytes_per_chunk; width and
 * height are those of the frames handed back (acquisition orientation);
 * chunk_pitch is the pitch of the reader's decoded-layer buffer; layer_slots 1. */
aqz_status aqz_reader_layout(const aqz_reader* r, aqz_level_layout* out);

/* Load a layer from n_frames frames lying back to back: frame i is bytes
 * [offsets[i], offsets[i + 1]) of `frames` and holds chunk chunk_of_frame[i]
 * of the layer (offsets: n_frames + 1 values, chunk_of_frame: n_frames; both
 * host arrays, read before the call returns).  chunk_of_frame == NULL: the
 * order aqz_stage_compress_layer writes (shard-major, aqz_stage_compressed_
 * entries), with n_frames == chunks_per_layer.  Chunks not listed, and
 * zero-length frames, are chunks never written.  mem: where `frames` lies --
 * AQZ_MEM_HOST and AQZ_MEM_HOST_PINNED are copied into the reader's staging
 * buffer (frames_bytes <= max_frames_bytes), AQZ_MEM_DEVICE is decoded in
 * place and must stay valid until the load has run on `stream`.
 * codec: the AQZ_CODEC_* the frames were written with.  AQZ_CODEC_NONE: a
 * frame is the chunk itself (bytes_per_chunk long, else its status is
 * AQZ_DECODE_BAD_HEADER); device frames are then borrowed until the next load.
 * Enqueued on `stream` (hipStream_t; NULL = default) behind the reads of the
 * previous layer enqueued so far, on whichever streams.
 * AQZ_STATUS_INVALID_ARGUMENT (with an aqz_last_error text): a chunk_of_frame
 * entry >= chunks_per_layer or listed twice, offsets that decrease or exceed
 * frames_bytes, a codec the reader was not created for.  A malformed frame is
 * a per-chunk status (aqz_reader_status), as in aqz_decompressor_run: the
 * other chunks' pixels are exact, and the pixels of the bad chunk are
 * unspecified but written only inside the destination frames. */
aqz_status aqz_reader_load_frames(aqz_reader* r, const void* frames, size_t frames_bytes,
                                  int32_t mem, const uint64_t* offsets,
                                  const uint32_t* chunk_of_frame, uint32_t n_frames,
                                  int32_t codec, void* stream);
/* Load a layer of decoded chunks already on the device (e.g. what
 * aqz_stage_device_layer returns): chunk c at chunks + c * pitch, pitch >=
 * bytes_per_chunk.  has_data (device) NULL = every chunk present, else chunk
 * c is present iff has_data[c] == tag.  Nothing is copied: the chunks are
 * borrowed until the next load. */
aqz_status aqz_reader_load_chunks(aqz_reader* r, const void* chunks, uint64_t pitch,
                                  const uint32_t* has_data, uint32_t tag, void* stream);
/* Frames [first, first + count) of the loaded layer (ids inside the layer, in
 * acquisition order) -> dst + i * dst_stride (device), row-major.  Only bytes
 * [0, frame_bytes) of each destination frame are written; dst_stride >=
 * frame_bytes, any alignment.  Enqueued on `stream` behind the load; returns
 * at once.  A range outside the layer or a dst_stride below frame_bytes is
 * AQZ_STATUS_INVALID_ARGUMENT. */
aqz_status aqz_reader_read_frames(aqz_reader* r, uint32_t first, uint32_t count, void* dst,
                                  uint64_t dst_stride, void* stream);
/* Waits for the last load.  status (chunks_per_layer values, may be NULL):
 * the AQZ_DECODE_* of every chunk by chunk index, AQZ_DECODE_SKIPPED for
 * chunks never written; *n_bad = chunks with an error status. */
aqz_status aqz_reader_status(aqz_reader* r, uint32_t* status, size_t cap, uint32_t* n_bad);

/* ---- region reads: a crop of a few frames, decoding only its chunks ---------
 * A region is in pixels of the frames the reader hands back (acquisition
 * orientation: the width / height of aqz_reader_layout).  It is valid when
 * width > 0, height > 0, x0 + width <= layout.width and y0 + height <=
 * layout.height, the sums taken in 64 bits. */
typedef struct
{
    uint32_t x0, y0, width, height;
} aqz_region;
#define AQZ_DECODE_NOT_LOADED 5 /* aqz_reader_status after aqz_reader_load_frames_region: the
                                   chunk lies outside the loaded window; not an error status */
/* The chunks of a layer that hold a pixel of `region` in frames [first, first +
 * count) (ids inside the layer, acquisition order, as aqz_reader_read_frames
 * takes them): ascending, each once, through transpose_frame_id and an
 * XY-swapped storage order of d.  Host only.  *n = the count needed, always;
 * chunks == NULL: count only; cap < *n: AQZ_STATUS_OVERFLOW.
 * AQZ_STATUS_INVALID_ARGUMENT (with an aqz_last_error text): an invalid
 * region, count == 0, a range outside aqz_dims_frames_per_chunk_layer, NULL
 * d, region or n. */
aqz_status aqz_dims_region_chunks(const aqz_dims* d, uint32_t first, uint32_t count,
                                  const aqz_region* region, uint32_t* chunks, size_t cap,
                                  uint32_t* n);
/* The same for a reader's own dims. */
aqz_status aqz_reader_region_chunks(const aqz_reader* r, uint32_t first, uint32_t count,
                                    const aqz_region* region, uint32_t* chunks, size_t cap,
                                    uint32_t* n);
/* aqz_reader_load_frames for the window (first, count, region) only; the
 * arguments mean the same and the load is ordered the same way.  Frames of
 * chunks outside aqz_reader_region_chunks(first, count, region) are neither
 * copied to the device nor decoded, their bytes are not read (offsets is
 * still checked whole), and their status is AQZ_DECODE_NOT_LOADED.  Chunks
 * inside the window behave as after aqz_reader_load_frames: a zero-length
 * frame or a chunk not listed is AQZ_DECODE_SKIPPED and reads as zeros.
 * The needed frames are packed back to back into the reader's staging buffer,
 * runs of adjacent frames in one copy each -- over PCIe for AQZ_MEM_HOST /
 * AQZ_MEM_HOST_PINNED, on the device for AQZ_MEM_DEVICE with a codec (stored
 * chunks, AQZ_CODEC_NONE, in device memory are borrowed where they lie) -- so
 * the limit is the sum of the needed frames' bytes <= max_frames_bytes, not
 * frames_bytes.  The reader remembers the window until the next load: a
 * read_region or read_frames whose chunks are not all inside it is
 * AQZ_STATUS_INVALID_ARGUMENT, the text names the window, and nothing is
 * enqueued (a chunk that was not loaded never reads as zeros silently). */
aqz_status aqz_reader_load_frames_region(aqz_reader* r, const void* frames, size_t frames_bytes,
                                         int32_t mem, const uint64_t* offsets,
                                         const uint32_t* chunk_of_frame, uint32_t n_frames,
                                         int32_t codec, uint32_t first, uint32_t count,
                                         const aqz_region* region, void* stream);
/* The crop of frames [first, first + count) of the loaded layer, after any
 * load: pixel (y0 + j, x0 + i) of frame first + k goes to dst + k *
 * dst_frame_stride + j * dst_row_stride + i * bytes_per_pixel (device).  Only
 * those width * bytes_per_pixel bytes of each of the height rows are written,
 * so dst may be a window of a larger canvas.  dst_row_stride >= width * bpp,
 * dst_frame_stride >= (height - 1) * dst_row_stride + width * bpp, any
 * alignment (16-byte units when x0 * bpp, width * bpp, both strides and dst
 * are multiples of 16, narrower ones otherwise).  Enqueued on `stream` behind
 * the load.  AQZ_STATUS_INVALID_ARGUMENT: NULL or invalid region, count == 0
 * or a range outside the layer, a stride too small, nothing loaded, chunks
 * outside the window of a region load. */
aqz_status aqz_reader_read_region(aqz_reader* r, uint32_t first, uint32_t count,
                                  const aqz_region* region, void* dst, uint64_t dst_row_stride,
                                  uint64_t dst_frame_stride, void* stream);

/* ---- window loads: decode only the blosc blocks a region read needs ----------
 * Every block of a blosc1 frame is compressed and shuffled on its own, and a
 * frame's tile inside a chunk is one contiguous run of bytes, so a crop of a few
 * frames needs a short byte interval of each of its chunks, and of the frame only
 * the blocks that meet it.  Chunk bytes [lo, hi). */
typedef struct
{
    uint64_t lo, hi;
} aqz_byte_range;
/* aqz_dims_region_chunks with, for chunks[i], ranges[i]: the smallest interval of
 * chunk bytes that holds every byte a crop of `region` from frames [first, first +
 * count) reads (0 <= lo < hi <= bytes_per_chunk), through transpose_frame_id and an
 * XY-swapped storage order.  Host only.  *n = the count needed, always; chunks or
 * ranges NULL: that array is not filled (both NULL: count only); cap < *n with an
 * array given: AQZ_STATUS_OVERFLOW.  The arguments are checked, and refused with the
 * texts, as aqz_dims_region_chunks does. */
aqz_status aqz_dims_region_chunk_ranges(const aqz_dims* d, uint32_t first, uint32_t count,
                                        const aqz_region* region, uint32_t* chunks,
                                        aqz_byte_range* ranges, size_t cap, uint32_t* n);
/* The same for a reader's own dims. */
aqz_status aqz_reader_region_chunk_ranges(const aqz_reader* r, uint32_t first, uint32_t count,
                                          const aqz_region* region, uint32_t* chunks,
                                          aqz_byte_range* ranges, size_t cap, uint32_t* n);
/* aqz_decompressor_run over chunk bytes ranges[i] of frame i only (ranges: device,
 * n_chunks entries; spans: device, n_chunks entries, may be NULL).  Per frame:
 *  - a blosc1 frame (LZ4 or zstd codec; any block size, split or not, any shuffle):
 *    only blocks [lo / blocksize, ceil(hi / blocksize)) are looked up in the block
 *    table, decoded and un-shuffled; spans[i] is the block-aligned interval
 *    [jlo * blocksize, min(jhi * blocksize, chunk_bytes)).  Of the frame, only the
 *    header, those blocks' table entries and their records are read: a defect
 *    elsewhere is not looked at and not reported; one inside gets the status a full
 *    decode gives it.
 *  - a memcpyed or zero-length frame: exactly [lo, hi) is copied or zero-filled;
 *    spans[i] = ranges[i].
 *  - a plain zstd frame is decoded whole (its matches reach across blocks), by the
 *    block-parallel kernels where the decoder has them; spans[i] = [0, chunk_bytes).
 *  - lo == hi: the frame is not decoded, status[i] = AQZ_DECODE_NOT_LOADED, empty
 *    span.  lo > hi or hi > chunk_bytes: status[i] = AQZ_DECODE_BAD_HEADER, empty
 *    span.  An empty span is {0, 0}; so is the span of a frame whose header is
 *    refused.
 * No byte of chunk i outside spans[i] is written. */
aqz_status aqz_decompressor_run_ranges(aqz_decompressor* d, const void* frames,
                                       size_t frames_bytes, const uint64_t* offsets,
                                       uint32_t n_chunks, void* dst, uint64_t pitch,
                                       uint64_t chunk_bytes, const aqz_byte_range* ranges,
                                       aqz_byte_range* spans, uint32_t* status, void* stream);
/* aqz_reader_load_frames_region, decoding only the window's bytes: the frames of
 * the window's chunks are copied and packed the same way (whole frames: the block
 * table is needed), each is decoded over its aqz_reader_region_chunk_ranges hull
 * only, and the chunks outside the window get an empty range -- they are neither
 * decoded nor zero-filled (AQZ_DECODE_NOT_LOADED).  The reader remembers the exact
 * window until the next load: a read_region or read_frames whose frames are not
 * inside [first, first + count) or whose region is not inside `region` is
 * AQZ_STATUS_INVALID_ARGUMENT, the text names the window, and nothing is enqueued
 * (a byte that was not decoded is never handed out).  Stored chunks
 * (AQZ_CODEC_NONE) are loaded as by the region load.  The first call on a reader
 * with codecs allocates 32 bytes per chunk of device memory (and as much pinned):
 * the ranges and the spans; aqz_reader_device_bytes does not count them. */
aqz_status aqz_reader_load_frames_window(aqz_reader* r, const void* frames, size_t frames_bytes,
                                         int32_t mem, const uint64_t* offsets,
                                         const uint32_t* chunk_of_frame, uint32_t n_frames,
                                         int32_t codec, uint32_t first, uint32_t count,
                                         const aqz_region* region, void* stream);
/* Waits for the last load.  *decoded_bytes: the chunk bytes its decoder wrote --
 * the sum of the spans of a window load; chunks_per_layer * bytes_per_chunk after
 * aqz_reader_load_frames or aqz_reader_load_frames_region with a codec (a region
 * load zero-fills the chunks outside its window); 0 for stored chunks and
 * aqz_reader_load_chunks.  *copied_bytes: the frame bytes it copied into the
 * staging buffer.  Either may be NULL. */
aqz_status aqz_reader_load_stats(aqz_reader* r, uint64_t* decoded_bytes, uint64_t* copied_bytes);

#ifdef __cplusplus
}
#endif
#endif /* AQZ_GPU_H */
