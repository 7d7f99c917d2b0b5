// aqz_zstdpar.hh -- the block-parallel shape of the device zstd decoder, on
// top of aqz_zstddec.hh's parse and compiled for host and device from this
// one text, as that file is.  A plain zstd frame is decoded in four phases:
//
//   (a) index    par_index: the frame header and the block-header walk into a
//                block table (Block); of a compressed block the literals
//                header, the sequence count, the modes byte and, for each of
//                the four tables (Huffman tree, LL, OF, ML), the block that
//                defines the table in effect (treeless literals and
//                Repeat_Mode chain back to it); prefix sums of the Huffman
//                literal sizes and of the sequence counts (scratch offsets).
//   (b) entropy  par_entropy: one block, independent of its neighbours: the
//                tables rebuilt from their defining blocks, the Huffman
//                streams decoded into the block's literal area, the FSE
//                sequence stream into Record{ll, ml, ov}, the block's
//                regenerated size.
//   (c) place    par_place / par_copy_block: the exclusive scan of the
//                regenerated sizes (their sum must be n_dst), and inside a
//                block the scan of ll + ml that gives every record its
//                output position.
//   (d) execute  par_copy_block: raw / RLE blocks and every literal run are
//                copies with known source and destination; par_matches: the
//                repeat offsets resolved in stream order (rep_step) and the
//                matches copied.
//
// The kernels (aqz_zstdpar.hip) run (a) and (b) from this text and redo the
// scans and movers of (c) and (d) with the lanes of a wave; the serial forms
// here are what tests/sanitize/zstdpar_sanitize.cpp runs under a host
// sanitizer and compares with zdec::zstd_decode_frame.
//
// Every error past the frame header is kCorrupt in zstd_decode_frame, so
// "the same status" means: this path refuses exactly the frames that one
// refuses.  Bounds that the serial walk checks against the running output
// position follow here from the sums: sizes only add up, and the total must
// be n_dst.
#pragma once

#include "aqz_zstddec.hh"

namespace aqz {
namespace zpar {

using dec::kCorrupt;
using dec::kOk;

constexpr uint32_t kNone = 0xffffffffu;

// Blocks the table of a chunk of n bytes holds.  libzstd cuts blocks of
// min(128 KiB, window) bytes and its smallest window is 1 KiB; this library's
// blocks are 8 KiB.  A frame with more blocks (empty or tiny ones, which no
// encoder at hand writes) is left to the serial decoder.
AQZ_ZINL uint32_t
block_capacity(uint64_t n)
{
    return uint32_t(n / 1024) + 16;
}
// Records a frame that decodes to n bytes can hold: a sequence regenerates
// at least 3 bytes.
AQZ_ZINL uint64_t
record_capacity(uint64_t n)
{
    return n / 3;
}

struct Block
{
    uint32_t pos;      // Block_Content within the frame
    uint32_t size;     // Block_Size
    uint32_t type;     // 0 raw, 1 RLE, 2 compressed
    uint32_t lit_type; // compressed: Literals_Block_Type
    uint32_t lit_n;    //   regenerated literals
    uint32_t lit_src;  //   raw literals: their position in the frame; RLE: the byte
    uint32_t lit_off;  //   Huffman literals: first byte in the frame's literal area
    uint32_t nseq;
    uint32_t seq_off;  //   first record in the frame's record area
    uint32_t seq_pos;  //   within the block: the byte after Symbol_Compression_Modes
    uint32_t def[4];   //   block that defines the Huffman tree / LL / OF / ML table in effect
    uint32_t regen;    // bytes the block regenerates ((a) raw, RLE; (b) compressed)
    uint32_t out;      // (c) first output byte
};

struct Record
{
    uint32_t ll; // (c) turns it into the match's output position
    uint32_t ml; // (c) adds kLl0 when ll == 0
    uint32_t ov; // Offset_Value
};
constexpr uint32_t kLl0 = 0x80000000u;

// The header of a literals section at b[0, n), with literals_section's checks.
struct LitHeader
{
    uint32_t type, sf, hdr, regen, comp;
    uint32_t used; // bytes of the whole section
};

AQZ_ZINL uint32_t
lit_header(const uint8_t* b, uint32_t n, uint32_t room, LitHeader& h)
{
    if (n < 1)
        return kCorrupt;
    const uint32_t b0 = b[0];
    h.type = b0 & 3u;
    h.sf = (b0 >> 2) & 3u;
    h.comp = 0;
    if (h.type < 2) {
        if (h.sf == 0 || h.sf == 2) {
            h.hdr = 1;
            h.regen = b0 >> 3;
        } else if (h.sf == 1) {
            if (n < 2)
                return kCorrupt;
            h.hdr = 2;
            h.regen = (b0 >> 4) | uint32_t(b[1]) << 4;
        } else {
            if (n < 3)
                return kCorrupt;
            h.hdr = 3;
            h.regen = (b0 >> 4) | uint32_t(b[1]) << 4 | uint32_t(b[2]) << 12;
        }
        if (h.regen > zdec::kBlockMax || h.regen > room)
            return kCorrupt;
        if (h.type == 0) {
            if (h.regen > n - h.hdr)
                return kCorrupt;
            h.used = h.hdr + h.regen;
        } else {
            if (n - h.hdr < 1)
                return kCorrupt;
            h.used = h.hdr + 1;
        }
        return kOk;
    }
    h.hdr = h.sf < 2 ? 3u : h.sf + 2u;
    const uint32_t bits = h.sf < 2 ? 10u : h.sf == 2 ? 14u : 18u;
    if (n < h.hdr)
        return kCorrupt;
    uint64_t v = 0;
    for (uint32_t k = 0; k < h.hdr; ++k)
        v |= uint64_t(b[k]) << (8 * k);
    v >>= 4;
    h.regen = uint32_t(v & ((1u << bits) - 1u));
    h.comp = uint32_t((v >> bits) & ((1u << bits) - 1u));
    if (h.regen > zdec::kBlockMax || h.regen > room || h.comp > n - h.hdr)
        return kCorrupt;
    h.used = h.hdr + h.comp;
    return kOk;
}

// ---- (a) index ------------------------------------------------------------------
// What the walk carries from block to block.
struct IndexState
{
    uint32_t def[4];
    uint32_t lit_all; // literals of every kind: all of them reach the output
    uint32_t lit_huf; // Huffman literals: the literal area
    uint64_t nseq;
};

AQZ_ZINL uint32_t
index_compressed(const uint8_t* f, uint32_t j, uint32_t n_dst, IndexState& s, Block& B)
{
    const uint8_t* b = f + B.pos;
    const uint32_t n = B.size;
    LitHeader h{};
    const uint32_t e = lit_header(b, n, n_dst, h);
    if (e != kOk)
        return e;
    B.lit_type = h.type;
    B.lit_n = h.regen;
    if (h.type == 0)
        B.lit_src = B.pos + h.hdr;
    else if (h.type == 1)
        B.lit_src = b[h.hdr];
    else {
        if (h.type == 2)
            s.def[0] = j;
        else if (s.def[0] == kNone)
            return kCorrupt; // nothing to repeat
        B.lit_off = s.lit_huf;
        s.lit_huf += h.regen;
    }
    s.lit_all += h.regen; // <= n_dst + kBlockMax: no wrap
    if (s.lit_all > n_dst)
        return kCorrupt;
    uint32_t p = h.used;
    if (p >= n)
        return kCorrupt;
    uint32_t nseq = b[p++];
    if (nseq >= 128) {
        if (nseq == 255) {
            if (n - p < 2)
                return kCorrupt;
            nseq = (b[p] | uint32_t(b[p + 1]) << 8) + 0x7F00u;
            p += 2;
        } else {
            if (n - p < 1)
                return kCorrupt;
            nseq = ((nseq - 128) << 8) + b[p++];
        }
    }
    B.nseq = nseq;
    if (nseq == 0) {
        if (p != n)
            return kCorrupt;
    } else {
        if (p >= n)
            return kCorrupt;
        const uint32_t modes = b[p++];
        if (modes & 3u)
            return kCorrupt;
        for (uint32_t w = 0; w < 3; ++w) {
            if (((modes >> (6 - 2 * w)) & 3u) != 3)
                s.def[1 + w] = j;
            else if (s.def[1 + w] == kNone)
                return kCorrupt; // nothing to repeat
        }
        B.seq_pos = p;
        B.seq_off = uint32_t(s.nseq);
        s.nseq += nseq;
        if (3 * s.nseq > n_dst)
            return kCorrupt;
    }
    for (uint32_t w = 0; w < 4; ++w)
        B.def[w] = s.def[w];
    return kOk;
}

// The block table of f[0, len), which must decode to n_dst bytes.  taken =
// false (and kOk): the frame has more than cap blocks and is left alone.
// nseq_total: the records of the frame.
AQZ_ZINL uint32_t
par_index(const uint8_t* f, uint32_t len, uint32_t n_dst, Block* tab, uint32_t cap,
          uint32_t& nblocks, uint32_t& nseq_total, bool& taken)
{
    taken = true;
    nblocks = 0;
    nseq_total = 0;
    zdec::FrameHeader h{};
    const uint32_t e = zdec::parse_frame_header(f, len, n_dst, h);
    if (e != kOk)
        return e;
    IndexState s{ { kNone, kNone, kNone, kNone }, 0, 0, 0 };
    uint32_t pos = h.header_bytes, j = 0;
    for (;;) {
        if (len - pos < 3)
            return kCorrupt;
        const uint32_t bh = f[pos] | uint32_t(f[pos + 1]) << 8 | uint32_t(f[pos + 2]) << 16;
        pos += 3;
        const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, size = bh >> 3;
        if (type == 3 || size > zdec::kBlockMax)
            return kCorrupt;
        if (j >= cap) {
            taken = false;
            return kOk;
        }
        Block B{};
        B.pos = pos;
        B.size = size;
        B.type = type;
        B.regen = size;
        if (type == 1) {
            if (len - pos < 1)
                return kCorrupt;
            pos += 1;
        } else {
            if (size > len - pos)
                return kCorrupt;
            if (type == 2) {
                B.regen = 0;
                const uint32_t eb = index_compressed(f, j, n_dst, s, B);
                if (eb != kOk)
                    return eb;
            }
            pos += size;
        }
        tab[j++] = B;
        if (last)
            break;
    }
    if (len - pos != h.checksum)
        return kCorrupt;
    nblocks = j;
    nseq_total = uint32_t(s.nseq);
    return kOk;
}

// ---- (b) block entropy decode ---------------------------------------------------
// Table w (0 LL, 1 OF, 2 ML) as block D describes it: D's descriptions are
// walked in order up to w.  D's mode for w is not Repeat_Mode (it defines w).
AQZ_ZINL uint32_t
load_seq_table(const uint8_t* f, const Block& D, uint32_t w, zdec::Tables& t)
{
    const uint8_t* b = f + D.pos;
    const uint32_t n = D.size;
    uint32_t p = D.seq_pos;
    const uint32_t modes = b[p - 1];
    for (uint32_t k = 0; k < w; ++k) {
        const uint32_t mode = (modes >> (6 - 2 * k)) & 3u;
        if (mode == 1) {
            if (p >= n)
                return kCorrupt;
            p += 1;
        } else if (mode == 2) {
            uint32_t log = 0, used = 0;
            const uint32_t e = zdec::fse_read_norm(
              b + p, n - p, k == 0 ? zdec::kLLMax : zdec::kOFMax,
              k == 0 ? zdec::kLLLog : zdec::kOFLog, t.norm, log, used);
            if (e != kOk)
                return e;
            if (used > n - p)
                return kCorrupt;
            p += used;
        }
    }
    const uint32_t mode = (modes >> (6 - 2 * w)) & 3u;
    if (mode == 3)
        return kCorrupt;
    return zdec::seq_table(b, n, p, mode, w, t);
}

//   io.huf(b, job, tab, log)   as zdec::literals_section asks: the Huffman
//                              streams into the block's literal area
//   io.record(i, ll, ml, ov)   record i of the frame
// regen: the bytes the block regenerates.
template<typename Io>
AQZ_ZINL uint32_t
par_entropy(Io& io, const uint8_t* f, const Block* tab, uint32_t j, uint32_t n_dst,
            zdec::Tables& t, uint32_t& regen)
{
    const Block& B = tab[j];
    const uint8_t* b = f + B.pos;
    const uint32_t n = B.size;
    t.huf_log = 0;
    t.have_ll = t.have_of = t.have_ml = 0;
    t.ll_log = t.of_log = t.ml_log = 0;
    if (B.lit_type == 3) { // treeless: the tree of the defining block
        const Block& D = tab[B.def[0]];
        LitHeader dh{};
        uint32_t e = lit_header(f + D.pos, D.size, n_dst, dh);
        if (e != kOk || dh.type != 2)
            return kCorrupt;
        uint32_t used = 0;
        e = zdec::huf_read_tree(f + D.pos + dh.hdr, dh.comp, t, used);
        if (e != kOk)
            return e;
    }
    zdec::Lits L{};
    uint32_t p = 0;
    uint32_t e = zdec::literals_section(io, b, B.pos, n, n_dst, t, L, p);
    if (e != kOk)
        return e;
    if (L.n != B.lit_n)
        return kCorrupt;
    if (B.nseq == 0) {
        regen = L.n;
        return kOk;
    }
    p = B.seq_pos;
    const uint32_t modes = b[p - 1];
    for (uint32_t w = 0; w < 3; ++w) {
        const uint32_t mode = (modes >> (6 - 2 * w)) & 3u;
        if (mode == 3)
            e = load_seq_table(f, tab[B.def[1 + w]], w, t);
        else
            e = zdec::seq_table(b, n, p, mode, w, t);
        if (e != kOk)
            return e;
    }
    zdec::BitR r;
    if (p >= n || !r.init(b + p, n - p))
        return kCorrupt;
    uint32_t sl = r.read(t.ll_log), so = r.read(t.of_log), sm = r.read(t.ml_log);
    if (r.pos < 0)
        return kCorrupt;
    uint32_t li = 0, msum = 0;
    for (uint32_t q = 0; q < B.nseq; ++q) {
        const zdec::FseEntry el = t.ll[sl], eo = t.of[so], em = t.ml[sm];
        const uint32_t ofc = eo.sym;
        if (ofc > zdec::kOFMax)
            return kCorrupt;
        const uint32_t ov = (1u << ofc) + r.read(ofc);
        uint32_t mbase, mnb, lbase, lnb;
        zdec::ml_base(em.sym <= zdec::kMLMax ? em.sym : zdec::kMLMax, mbase, mnb);
        zdec::ll_base(el.sym <= zdec::kLLMax ? el.sym : zdec::kLLMax, lbase, lnb);
        const uint32_t ml = mbase + r.read(mnb);
        const uint32_t ll = lbase + r.read(lnb);
        if (q + 1 < B.nseq) {
            sl = el.base + r.read(el.nb);
            sm = em.base + r.read(em.nb);
            so = eo.base + r.read(eo.nb);
        }
        if (r.pos < 0)
            return kCorrupt;
        if (ll > L.n - li)
            return kCorrupt;
        li += ll;
        msum += ml; // <= n_dst + 2^18: no wrap
        if (msum > n_dst)
            return kCorrupt;
        io.record(B.seq_off + q, ll, ml, ov);
    }
    if (r.pos != 0)
        return kCorrupt;
    regen = L.n + msum;
    return kOk;
}

// ---- (c) placement --------------------------------------------------------------
AQZ_ZINL uint32_t
par_place(Block* tab, uint32_t nblocks, uint32_t n_dst)
{
    uint64_t d = 0;
    for (uint32_t j = 0; j < nblocks; ++j) {
        tab[j].out = uint32_t(d);
        d += tab[j].regen;
        if (d > n_dst)
            return kCorrupt;
    }
    return d == n_dst ? kOk : kCorrupt;
}

// ---- (d) execute ----------------------------------------------------------------
// The offset of a sequence and the repeat offsets after it (RFC 8878 3.1.1.5).
AQZ_ZINL uint32_t
rep_step(zdec::FrameState& fs, uint32_t ov, bool ll0)
{
    uint32_t off;
    if (ov > 3) {
        off = ov - 3;
        fs.rep2 = fs.rep1;
        fs.rep1 = fs.rep0;
        fs.rep0 = off;
    } else {
        const uint32_t idx = ov + (ll0 ? 1u : 0u); // 1..4
        if (idx == 1) {
            off = fs.rep0;
        } else {
            off = idx == 2 ? fs.rep1 : idx == 3 ? fs.rep2 : fs.rep0 - 1;
            if (idx != 2)
                fs.rep2 = fs.rep1;
            fs.rep1 = fs.rep0;
            fs.rep0 = off;
        }
    }
    return off;
}

// Serial forms of (c) inside a block and of (d), with zdec's movers:
//   io.copy_src(d, q, n) / io.copy_lit(d, i, n) / io.fill(d, v, n) /
//   io.match(d, off, n); copy_lit's i counts from the frame's literal area.
// One block: its records placed, its raw / RLE bytes and literal runs copied.
template<typename Io>
AQZ_ZINL void
par_copy_block(Io& io, const uint8_t* f, const Block& B, Record* rec)
{
    if (B.type == 0) {
        if (B.size)
            io.copy_src(B.out, B.pos, B.size);
        return;
    }
    if (B.type == 1) {
        if (B.size)
            io.fill(B.out, f[B.pos], B.size);
        return;
    }
    uint32_t d = B.out, li = 0;
    for (uint32_t q = 0; q <= B.nseq; ++q) {
        uint32_t ll = B.lit_n - li; // after the last sequence: the rest
        if (q < B.nseq) {
            Record& r = rec[B.seq_off + q];
            ll = r.ll;
            r.ll = d + ll;
            r.ml |= ll == 0 ? kLl0 : 0u;
        }
        if (ll) {
            if (B.lit_type == 0)
                io.copy_src(d, B.lit_src + li, ll);
            else if (B.lit_type == 1)
                io.fill(d, B.lit_src, ll);
            else
                io.copy_lit(d, B.lit_off + li, ll);
        }
        li += ll;
        d += ll;
        if (q < B.nseq)
            d += rec[B.seq_off + q].ml & ~kLl0;
    }
}

// The match chain of the frame's placed records.
template<typename Io>
AQZ_ZINL uint32_t
par_matches(Io& io, const Record* rec, uint32_t nseq)
{
    zdec::FrameState fs{ 1, 4, 8 };
    for (uint32_t q = 0; q < nseq; ++q) {
        const Record r = rec[q];
        const uint32_t off = rep_step(fs, r.ov, (r.ml & kLl0) != 0);
        if (off == 0 || off > r.ll)
            return kCorrupt;
        io.match(r.ll, off, r.ml & ~kLl0);
    }
    return kOk;
}

} // namespace zpar
} // namespace aqz
