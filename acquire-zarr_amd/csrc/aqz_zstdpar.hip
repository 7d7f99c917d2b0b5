// aqz_zstdpar.hip -- the block-parallel decode of plain zstd frames on gfx950
// (AQZ_DECODE_ZSTD_PARALLEL).  The parse, the phases and every bound:
// aqz_zstdpar.hh (shared with the host).  The phases are kernels on the
// stream; nothing is handed from workgroup to workgroup inside a launch.
//
//   zstd_index    one workgroup per frame, lane 0: zpar::par_index.  The
//                 frame's word zfr[2q] becomes 0 (left to zstd_decode: not a
//                 plain zstd frame, or more blocks than the table holds) or
//                 1 + blocks; a malformed frame gets its status here.
//   zstd_entropy  grid (frame, block), one wave per block: zpar::par_entropy
//                 with the tables in LDS, the Huffman streams on four lanes,
//                 the sequence decode wave-uniform, records stored by lane 0.
//   zstd_place    one wave per frame: the scan of the regenerated sizes.
//   zstd_copy     grid (frame, block), one wave per block: raw and RLE
//                 blocks; of a compressed block the scan of ll + ml over
//                 batches of 64 records (a record becomes {match position,
//                 ml, ov}) and the literal runs, a lane per byte.
//   zstd_matches  one wave per frame: the records in batches of 64, one per
//                 lane.  The repeat offsets are resolved in stream order with
//                 wave-uniform scalars.  Then rounds: every pending match
//                 whose source ends at or before the first pending match's
//                 destination depends on no pending match; those are copied
//                 together, a lane per byte, and a workgroup-scope fence ends
//                 the round (later rounds and batches re-read those bytes).
//
// Output goes where zstd_decode would put it: the destination chunk, or the
// chunk's scratch slot in compare mode (zstd_finish compares it).
#include "aqz_decode.hh"
#include "aqz_decode_dev.hh"
#include "aqz_zstdpar.hh"

namespace aqz {
namespace {

struct Slot
{
    zpar::Block* tab;
    uint8_t* lit;
    zpar::Record* rec;
};

__device__ __forceinline__ Slot
slot_of(const DecodeParams& p, uint32_t q)
{
    uint8_t* s = p.zpar + uint64_t(q) * p.zpar_pitch;
    return Slot{ reinterpret_cast<zpar::Block*>(s), s + p.zpar_lit_off,
                 reinterpret_cast<zpar::Record*>(s + p.zpar_rec_off) };
}

// Frame q where the index took it and nothing has refused it: its blocks.
__device__ __forceinline__ uint32_t
taken_blocks(const DecodeParams& p, uint32_t q, FrameRef& r)
{
    const uint32_t w = p.zfr[2 * q];
    if (w <= 1 || p.status[q] != dec::kOk || !frame_ref(p, q, r))
        return 0;
    return w - 1;
}

__device__ __forceinline__ uint8_t*
out_of(const DecodeParams& p, uint32_t q, const FrameRef& r)
{
    return p.bad ? p.scratch + uint64_t(q) * p.scratch_pitch : r.out;
}

__global__ void __launch_bounds__(64)
zstd_index(DecodeParams p)
{
    const uint32_t q = blockIdx.x;
    if (threadIdx.x != 0)
        return;
    p.zfr[2 * q] = 0;
    p.zfr[2 * q + 1] = 0;
    FrameRef r;
    if (!frame_ref(p, q, r) || r.len == 0 || dec::frame_family(r.f, r.len) != dec::kFamilyZstd)
        return;
    const uint32_t magic = dec::rd32(r.f);
    if (magic != dec::kZstdMagic && (magic & 0xfffffff0u) != dec::kSkippableMagic) {
        atomicAdd(&p.zcounts[1], 1u); // a blosc1-zstd frame: zstd_decode's
        return;
    }
    const Slot s = slot_of(p, q);
    uint32_t cap = zpar::block_capacity(p.chunk_bytes);
    cap = cap < p.zpar_cap ? cap : p.zpar_cap;
    uint32_t nblocks = 0, nseq = 0;
    bool taken = false;
    const uint32_t e = zpar::par_index(r.f, uint32_t(r.len), uint32_t(p.chunk_bytes), s.tab, cap,
                                       nblocks, nseq, taken);
    if (!taken) {
        atomicAdd(&p.zcounts[1], 1u);
        return;
    }
    atomicAdd(&p.zcounts[0], 1u);
    if (e != dec::kOk) {
        atomicMax(&p.status[q], e);
        nblocks = 0;
    }
    p.zfr[2 * q] = 1 + nblocks;
    p.zfr[2 * q + 1] = nseq;
}

// The movers of par_entropy for one wave.
struct WaveEIo
{
    uint8_t* lit;       // the block's literal area
    zpar::Record* rec;  // the frame's records
    uint32_t lane;

    __device__ __forceinline__ uint32_t huf(const uint8_t* f, const zdec::HufJob& j,
                                            const uint16_t* tab, uint32_t log)
    {
        uint32_t e = dec::kOk;
        if (lane < j.ns) {
            const uint32_t k = lane;
            const uint32_t src = k == 0 ? j.src[0] : k == 1 ? j.src[1] : k == 2 ? j.src[2] : j.src[3];
            const uint32_t len = k == 0 ? j.len[0] : k == 1 ? j.len[1] : k == 2 ? j.len[2] : j.len[3];
            const uint32_t dst = k == 0 ? j.dst[0] : k == 1 ? j.dst[1] : k == 2 ? j.dst[2] : j.dst[3];
            const uint32_t cnt = k == 0 ? j.cnt[0] : k == 1 ? j.cnt[1] : k == 2 ? j.cnt[2] : j.cnt[3];
            e = zdec::huf_decode_stream(f + src, len, tab, log, lit + dst, cnt);
        }
        uint32_t worst = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ek = uint32_t(__builtin_amdgcn_readlane(int(e), k));
            worst = ek > worst ? ek : worst;
        }
        return worst;
    }

    __device__ __forceinline__ void record(uint32_t i, uint32_t ll, uint32_t ml, uint32_t ov)
    {
        if (lane == 0)
            rec[i] = zpar::Record{ ll, ml, ov };
    }
};

__global__ void __launch_bounds__(64)
zstd_entropy(DecodeParams p)
{
    __shared__ zdec::Tables s_t;
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    const uint32_t nb = taken_blocks(p, q, r);
    const Slot s = slot_of(p, q);
    uint32_t done = 0;
    for (uint32_t j = blockIdx.y; j < nb; j += gridDim.y) {
        if (s.tab[j].type != 2)
            continue;
        WaveEIo io{ s.lit + s.tab[j].lit_off, s.rec, lane };
        uint32_t regen = 0;
        const uint32_t e =
          zpar::par_entropy(io, r.f, s.tab, j, uint32_t(p.chunk_bytes), s_t, regen);
        if (lane == 0) {
            if (e != dec::kOk)
                atomicMax(&p.status[q], e);
            s.tab[j].regen = e == dec::kOk ? regen : 0u;
        }
        ++done;
    }
    if (done && lane == 0)
        atomicAdd(&p.zcounts[2], done);
}

// inclusive scan over the wave
__device__ __forceinline__ uint32_t
wave_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t u = uint32_t(__shfl_up(int(v), d, 64));
        if (lane >= d)
            v += u;
    }
    return v;
}

__global__ void __launch_bounds__(64)
zstd_place(DecodeParams p)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    const uint32_t nb = taken_blocks(p, q, r);
    if (nb == 0)
        return;
    const Slot s = slot_of(p, q);
    const uint32_t n_dst = uint32_t(p.chunk_bytes);
    // sizes are clamped to n_dst + 1, so a wave's sum stays below 2^38 / 64
    uint64_t base = 0;
    bool bad = false;
    for (uint32_t j0 = 0; j0 < nb && !bad; j0 += 64) {
        const uint32_t j = j0 + lane;
        uint32_t v = j < nb ? s.tab[j].regen : 0u;
        if (v > n_dst) {
            v = n_dst + 1;
        }
        // two 32-bit scans of the halves of a 38-bit sum: scan the value in
        // 64 bits by splitting into low 16 and high bits
        const uint32_t lo = wave_scan(v & 0xffffu, lane);
        const uint32_t hi = wave_scan(v >> 16, lane);
        const uint64_t incl = base + lo + (uint64_t(hi) << 16);
        const uint64_t excl = incl - v;
        if (j < nb)
            s.tab[j].out = uint32_t(excl > n_dst ? n_dst : excl);
        const uint64_t total = uint64_t(__shfl(int(uint32_t(incl)), 63, 64)) |
                               uint64_t(uint32_t(__shfl(int(uint32_t(incl >> 32)), 63, 64))) << 32;
        base = total;
        bad = base > n_dst;
    }
    if ((bad || base != n_dst) && lane == 0)
        atomicMax(&p.status[q], uint32_t(dec::kCorrupt));
}

// o[0, n) = s[0, n) by the wave, four loads in flight per lane
__device__ __forceinline__ void
wave_copy(uint8_t* o, const uint8_t* s, uint32_t n, uint32_t lane)
{
    for (uint32_t i = lane; i < n; i += 256) {
        const bool b1 = i + 64 < n, b2 = i + 128 < n, b3 = i + 192 < n;
        const uint8_t v0 = s[i];
        const uint8_t v1 = b1 ? s[i + 64] : uint8_t(0);
        const uint8_t v2 = b2 ? s[i + 128] : uint8_t(0);
        const uint8_t v3 = b3 ? s[i + 192] : uint8_t(0);
        o[i] = v0;
        if (b1)
            o[i + 64] = v1;
        if (b2)
            o[i + 128] = v2;
        if (b3)
            o[i + 192] = v3;
    }
}

// first k in [0, 64) with incl[k] > t (t below incl[63])
__device__ __forceinline__ uint32_t
find_run(const uint32_t* incl, uint32_t t)
{
    uint32_t k = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1)
        if (incl[k + step - 1] <= t)
            k += step;
    return k;
}

__global__ void __launch_bounds__(64)
zstd_copy(DecodeParams p)
{
    __shared__ uint32_t s_incl[64]; // inclusive sums of ll over the batch
    __shared__ uint32_t s_dst[64];  // output position of each record's literals
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    const uint32_t nb = taken_blocks(p, q, r);
    if (nb == 0)
        return;
    const Slot s = slot_of(p, q);
    uint8_t* out = out_of(p, q, r);
    for (uint32_t j = blockIdx.y; j < nb; j += gridDim.y) {
        const zpar::Block B = s.tab[j];
        if (B.type == 0) {
            wave_copy(out + B.out, r.f + B.pos, B.size, lane);
            continue;
        }
        if (B.type == 1) {
            const uint8_t v = r.f[B.pos];
            for (uint32_t i = lane; i < B.size; i += 64)
                out[B.out + i] = v;
            continue;
        }
        // literal i of the block
        const uint8_t* lsrc = B.lit_type == 0 ? r.f + B.lit_src : s.lit + B.lit_off;
        const bool rle = B.lit_type == 1;
        const uint8_t rle_byte = uint8_t(B.lit_src);
        uint32_t d = B.out, li = 0;
        for (uint32_t q0 = 0; q0 < B.nseq; q0 += 64) {
            const uint32_t i = q0 + lane;
            const bool have = i < B.nseq;
            zpar::Record rc{ 0, 0, 0 };
            if (have)
                rc = s.rec[B.seq_off + i];
            // sums stay within the block's regenerated size (<= n_dst)
            const uint32_t incl_ll = wave_scan(rc.ll, lane);
            const uint32_t incl_all = wave_scan(rc.ll + rc.ml, lane);
            const uint32_t dlit = d + incl_all - rc.ll - rc.ml;
            if (have) {
                rc.ml |= rc.ll == 0 ? zpar::kLl0 : 0u;
                s.rec[B.seq_off + i] = zpar::Record{ dlit + rc.ll, rc.ml, rc.ov };
            }
            __syncthreads(); // the last batch's readers are done
            s_incl[lane] = incl_ll;
            s_dst[lane] = dlit - (incl_ll - rc.ll); // + t: where literal t of the batch goes
            __syncthreads();
            const uint32_t total = s_incl[63];
            for (uint32_t t0 = lane; t0 < total; t0 += 256) {
                uint8_t v[4];
                uint32_t at[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint32_t t = t0 + 64 * u;
                    at[u] = 0;
                    v[u] = 0;
                    if (t < total) {
                        at[u] = s_dst[find_run(s_incl, t)] + t;
                        v[u] = rle ? rle_byte : lsrc[li + t];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u)
                    if (t0 + 64 * u < total)
                        out[at[u]] = v[u];
            }
            d += uint32_t(__shfl(int(incl_all), 63, 64));
            li += total;
        }
        // the literals after the last sequence
        const uint32_t rest = B.lit_n - li;
        if (rle) {
            for (uint32_t i = lane; i < rest; i += 64)
                out[d + i] = rle_byte;
        } else {
            wave_copy(out + d, lsrc + li, rest, lane);
        }
    }
}

__global__ void __launch_bounds__(64)
zstd_matches(DecodeParams p)
{
    __shared__ uint32_t s_incl[64]; // inclusive sums of the round's match lengths
    __shared__ uint32_t s_d[64];
    __shared__ uint32_t s_off[64];
    const uint32_t lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    FrameRef r;
    if (taken_blocks(p, q, r) == 0)
        return;
    const Slot s = slot_of(p, q);
    uint8_t* out = out_of(p, q, r);
    const uint32_t nseq = uni(p.zfr[2 * q + 1]);
    zdec::FrameState fs{ 1, 4, 8 };
    zpar::Record nxt{ 0, 0, 0 };
    if (lane < nseq)
        nxt = s.rec[lane];
    bool corrupt = false;
    for (uint32_t q0 = 0; q0 < nseq && !corrupt; q0 += 64) {
        const zpar::Record rc = nxt;
        const uint32_t cnt = nseq - q0 < 64 ? nseq - q0 : 64;
        if (q0 + 64 + lane < nseq) // the next batch, in flight behind this one
            nxt = s.rec[q0 + 64 + lane];
        // repeat offsets in stream order: wave-uniform scalars
        uint32_t off = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t ov = uint32_t(__builtin_amdgcn_readlane(int(rc.ov), k));
            const uint32_t ml = uint32_t(__builtin_amdgcn_readlane(int(rc.ml), k));
            const uint32_t o = zpar::rep_step(fs, ov, (ml & zpar::kLl0) != 0);
            if (lane == k)
                off = o;
        }
        const bool have = lane < cnt;
        const uint32_t d = rc.ll, ml = rc.ml & ~zpar::kLl0;
        if (__ballot(have && (off == 0 || off > d)) != 0) {
            corrupt = true;
            break;
        }
        // bytes read: out[d - off, d - off + min(ml, off))
        const uint32_t src_end = d - off + (ml < off ? ml : off);
        uint64_t pending = __ballot(have);
        while (pending) {
            const uint32_t first = uint32_t(__builtin_ctzll(pending));
            const uint32_t dmin = uint32_t(__builtin_amdgcn_readlane(int(d), first));
            const bool ready = ((pending >> lane) & 1ull) && src_end <= dmin;
            const uint32_t n = ready ? ml : 0u;
            // match lengths of a frame sum to at most n_dst: no wrap
            const uint32_t incl = wave_scan(n, lane);
            __syncthreads();
            s_incl[lane] = incl;
            s_d[lane] = d - (incl - n); // + t: where byte t of the round goes
            s_off[lane] = off;
            __syncthreads();
            const uint32_t total = s_incl[63];
            for (uint32_t t0 = lane; t0 < total; t0 += 256) {
                uint8_t v[4];
                uint32_t at[4];
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u) {
                    const uint32_t t = t0 + 64 * u;
                    at[u] = 0;
                    v[u] = 0;
                    if (t < total) {
                        const uint32_t k = find_run(s_incl, t);
                        const uint32_t o = s_off[k];
                        at[u] = s_d[k] + t;
                        // byte i of match k: out[d + i] = out[d - off + i % off]
                        const uint32_t first_t = k ? s_incl[k - 1] : 0u;
                        uint32_t i = t - first_t;
                        const uint32_t dk = at[u] - i;
                        if (i >= o)
                            i %= o;
                        v[u] = out[dk - o + i];
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < 4; ++u)
                    if (t0 + 64 * u < total)
                        out[at[u]] = v[u];
            }
            // stores of this round before the loads of the next
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            pending &= ~__ballot(ready);
        }
    }
    if (lane == 0) {
        if (corrupt)
            atomicMax(&p.status[q], uint32_t(dec::kCorrupt));
        atomicAdd(&p.zcounts[3], nseq);
    }
}

} // namespace

ZstdParLayout
zstd_parallel_layout(uint64_t max_chunk_bytes)
{
    ZstdParLayout l{};
    l.cap = zpar::block_capacity(max_chunk_bytes);
    l.lit_off = uint64_t(l.cap) * sizeof(zpar::Block);
    l.rec_off = l.lit_off + ((max_chunk_bytes + 15) & ~uint64_t(15));
    l.pitch = l.rec_off +
              ((zpar::record_capacity(max_chunk_bytes) * sizeof(zpar::Record) + 15) & ~uint64_t(15));
    return l;
}

uint64_t
zstd_parallel_bytes(uint64_t max_chunk_bytes, uint32_t max_chunks)
{
    return zstd_parallel_layout(max_chunk_bytes).pitch * max_chunks +
           ((uint64_t(max_chunks) * 8 + 15) & ~uint64_t(15)) + 16;
}

hipError_t
launch_zstd_parallel(const DecodeParams& p, hipStream_t stream)
{
    if (p.n_chunks == 0)
        return hipSuccess;
    if (!p.zfr || !p.zcounts || !p.zpar || !p.scratch || p.scratch_pitch < p.chunk_bytes ||
        p.zpar_cap == 0)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p.zcounts, 0, 16, stream);
    if (e != hipSuccess)
        return e;
    uint32_t gx = zpar::block_capacity(p.chunk_bytes);
    gx = gx < p.zpar_cap ? gx : p.zpar_cap;
    gx = gx < 2048 ? gx : 2048;
    const dim3 blocks(p.n_chunks, gx); // x: the frame (the larger limit), y: its blocks
    hipLaunchKernelGGL(zstd_index, dim3(p.n_chunks), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(zstd_entropy, blocks, dim3(64), 0, stream, p);
    hipLaunchKernelGGL(zstd_place, dim3(p.n_chunks), dim3(64), 0, stream, p);
    hipLaunchKernelGGL(zstd_copy, blocks, dim3(64), 0, stream, p);
    hipLaunchKernelGGL(zstd_matches, dim3(p.n_chunks), dim3(64), 0, stream, p);
    return hipGetLastError();
}

} // namespace aqz
