// aqz_zstddec.hh -- the zstd frame parser (RFC 8878) of the device decoder
// (aqz_zstddec.hip), compiled for host and device from this one text, as
// aqz_lz4dec.hh is: the frame header and block walk, the literals and
// sequences section headers, the Huffman weight decode and table build, the
// FSE distribution read and table build, the backward bit reader, the
// sequence decode, the repeat-offset state machine, and every bound.  Only
// the bulk byte movers differ (the Io argument of zstd_decode_frame): serial
// loops on the host (tests/sanitize/zstddec_sanitize.cpp runs this text under
// a host sanitizer), the 64 lanes of a wave on the device.
//
// Accepted: any conforming frame without a dictionary -- Single_Segment or a
// window descriptor, Frame_Content_Size of 0/1/2/4/8 bytes, a content
// checksum (its 4 bytes are accounted for, NOT verified), Raw / RLE /
// Compressed blocks of up to 128 KiB, all four literal kinds in 1 or 4
// streams, all four table modes for LL / OF / ML, repeat offsets.  Matches
// may reach back to any earlier byte of the frame.
//
// A malformed frame is a status, never a fault: every source read is
// checked against the frame's end, every output write against n_dst, every
// literal write against the regenerated size (<= 128 KiB), and table sizes
// follow from accuracy logs that are checked before a table is indexed.
#pragma once

#include "aqz_lz4dec.hh"

// one body per kernel: the small structs passed by reference stay in registers
#define AQZ_ZINL AQZ_HD inline __attribute__((always_inline))

namespace aqz {
namespace zdec {

using dec::kBadHeader;
using dec::kCorrupt;
using dec::kOk;
using dec::kUnsupported;

constexpr uint32_t kBlockMax = 128 * 1024; // block content and regenerated size
constexpr uint32_t kHufLog = 11;           // longest Huffman code
constexpr uint32_t kWeightLog = 6;         // FSE accuracy of Huffman weights
constexpr uint32_t kLLLog = 9, kOFLog = 8, kMLLog = 9;
constexpr uint32_t kLLMax = 35, kOFMax = 31, kMLMax = 52;

AQZ_ZINL uint32_t
highbit(uint32_t v) // v > 0
{
    return 31u - uint32_t(__builtin_clz(v));
}

// ---- tables -----------------------------------------------------------------
struct FseEntry
{
    uint16_t base; // next state = base + read(nb)
    uint8_t sym;
    uint8_t nb;
};

// Everything a frame's blocks share; a few KiB (LDS on the device).
struct Tables
{
    uint16_t huf[1u << kHufLog]; // symbol | bits << 8, indexed by huf_log bits
    FseEntry ll[1u << kLLLog];
    FseEntry of[1u << kOFLog];
    FseEntry ml[1u << kMLLog];
    FseEntry wt[1u << kWeightLog];
    uint8_t weights[256];
    int16_t norm[64];
    uint16_t next[64];
    uint32_t rank[kHufLog + 2];
    uint32_t huf_log;                // 0: no tree yet
    uint32_t ll_log, of_log, ml_log; // valid when the have_ flag is set
    uint32_t have_ll, have_of, have_ml;
};

// the predefined distributions (RFC 8878 3.1.1.3.2.2; the encoder's copies
// sit in aqz_zstd.hh, which needs the HIP headers)
AQZ_ZINL int32_t
ll_default(uint32_t s)
{
    static constexpr int8_t v[36] = { 4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2,
                               2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1 };
    return v[s];
}
AQZ_ZINL int32_t
ml_default(uint32_t s)
{
    static constexpr int8_t v[53] = { 1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                               1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                               1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1 };
    return v[s];
}
AQZ_ZINL int32_t
of_default(uint32_t s)
{
    static constexpr int8_t v[29] = { 1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1,
                               1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1 };
    return v[s];
}

// code -> baseline, extra bits
AQZ_ZINL void
ll_base(uint32_t c, uint32_t& base, uint32_t& nb)
{
    static constexpr uint32_t b[20] = { 16, 18, 20, 22, 24, 28, 32, 40, 48, 64,
                                 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536 };
    static constexpr uint8_t e[20] = { 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
    if (c < 16) {
        base = c;
        nb = 0;
    } else {
        base = b[c - 16];
        nb = e[c - 16];
    }
}
AQZ_ZINL void
ml_base(uint32_t c, uint32_t& base, uint32_t& nb)
{
    static constexpr uint32_t b[21] = { 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99,
                                 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539 };
    static constexpr uint8_t e[21] = { 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
    if (c < 32) {
        base = c + 3;
        nb = 0;
    } else {
        base = b[c - 32];
        nb = e[c - 32];
    }
}

// ---- bit readers --------------------------------------------------------------
// Backward reader over s[0, n): the last byte holds the end mark (its highest
// set bit); bits are taken from the top down.  pos = unread bits; a read
// below bit 0 gives zeros and leaves pos negative (the caller's error).
struct BitR
{
    const uint8_t* s;
    uint32_t n;
    int32_t pos;
    uint64_t win;   // bytes [wbase, wbase + 8) of s, zeros past n
    uint32_t wbase; // 0xffffffff: nothing loaded

    AQZ_ZINL bool init(const uint8_t* src, uint32_t len)
    {
        s = src;
        n = len;
        wbase = 0xffffffffu;
        win = 0;
        pos = 0;
        if (len == 0 || len > 0x0fffffffu || src[len - 1] == 0)
            return false;
        pos = int32_t((len - 1) * 8 + highbit(src[len - 1]));
        return true;
    }
    // bits [p, p + nb) of the stream, p >= 0, nb <= 32
    AQZ_ZINL uint32_t at(uint32_t p, uint32_t nb)
    {
        const uint32_t byte = p >> 3;
        if (byte < wbase || byte + 5 > wbase + 8) {
            wbase = byte >= 3 ? byte - 3 : 0;
            uint64_t w = 0;
            for (uint32_t k = 0; k < 8; ++k)
                if (wbase + k < n)
                    w |= uint64_t(s[wbase + k]) << (8 * k);
            win = w;
        }
        const uint64_t v = win >> (p - 8 * wbase);
        return uint32_t(v & ((1ull << nb) - 1ull));
    }
    // the nb bits below pos (zeros below bit 0); pos is not moved
    AQZ_ZINL uint32_t peek(uint32_t nb)
    {
        const int32_t p = pos - int32_t(nb);
        if (p >= 0)
            return nb ? at(uint32_t(p), nb) : 0u;
        if (pos <= 0)
            return 0;
        return at(0, uint32_t(pos)) << uint32_t(-p);
    }
    AQZ_ZINL uint32_t read(uint32_t nb)
    {
        const uint32_t v = peek(nb);
        pos -= int32_t(nb);
        return v;
    }
};

// Forward reader of an FSE distribution.
struct FwdR
{
    const uint8_t* s;
    uint32_t n;
    uint32_t pos; // bits
    bool over;
    AQZ_ZINL uint32_t read(uint32_t nb) // nb <= 16
    {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t b = (pos >> 3) + k;
            if (b < n)
                v |= uint32_t(s[b]) << (8 * k);
        }
        v = (v >> (pos & 7u)) & ((1u << nb) - 1u);
        pos += nb;
        if (pos > 8 * n)
            over = true;
        return v;
    }
};

// ---- FSE ----------------------------------------------------------------------
// The distribution at s[0, n) for symbols 0..max_sym: norm[] (-1 = "less than
// 1"), its accuracy log and the bytes it takes.  norm has max_sym + 1 <= 64
// entries.
AQZ_ZINL uint32_t
fse_read_norm(const uint8_t* s, uint32_t n, uint32_t max_sym, uint32_t max_log, int16_t* norm,
              uint32_t& log, uint32_t& used)
{
    FwdR r{ s, n, 0, false };
    log = r.read(4) + 5;
    if (r.over || log > max_log)
        return kCorrupt;
    int32_t remaining = int32_t(1u << log) + 1;
    int32_t threshold = int32_t(1u << log);
    uint32_t nbits = log + 1;
    uint32_t sym = 0;
    bool prev0 = false;
    while (remaining > 1 && sym <= max_sym) {
        if (prev0) {
            for (;;) {
                const uint32_t rep = r.read(2);
                if (r.over)
                    return kCorrupt;
                for (uint32_t k = 0; k < rep; ++k) {
                    if (sym > max_sym)
                        return kCorrupt;
                    norm[sym++] = 0;
                }
                if (rep != 3)
                    break;
            }
            prev0 = false;
            continue;
        }
        const int32_t max = (2 * threshold - 1) - remaining;
        int32_t count = int32_t(r.read(nbits - 1));
        if (count >= max) {
            count |= int32_t(r.read(1)) << (nbits - 1);
            if (count >= threshold)
                count -= max;
        }
        if (r.over)
            return kCorrupt;
        --count;
        remaining -= count < 0 ? -count : count;
        if (remaining < 1)
            return kCorrupt;
        norm[sym++] = int16_t(count);
        prev0 = count == 0;
        while (remaining < threshold) {
            --nbits;
            threshold >>= 1;
        }
    }
    if (remaining != 1)
        return kCorrupt;
    for (; sym <= max_sym; ++sym)
        norm[sym] = 0;
    used = (r.pos + 7) / 8;
    return kOk;
}

// The decoding table of a distribution that sums to 1 << log (log <= 9,
// nsym <= 64).  t has 1 << log entries.
AQZ_ZINL uint32_t
fse_build(FseEntry* t, const int16_t* norm, uint32_t nsym, uint32_t log, uint16_t* next)
{
    const uint32_t size = 1u << log;
    uint32_t high = size; // one past the last free cell
    uint32_t total = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        if (norm[s] == -1) {
            if (high == 0)
                return kCorrupt;
            t[--high].sym = uint8_t(s);
            next[s] = 1;
            total += 1;
        } else {
            next[s] = uint16_t(norm[s]);
            total += uint32_t(norm[s]);
        }
    }
    if (total != size)
        return kCorrupt;
    const uint32_t step = (size >> 1) + (size >> 3) + 3, mask = size - 1;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < nsym; ++s) {
        for (int32_t i = 0; i < norm[s]; ++i) {
            t[pos].sym = uint8_t(s);
            do
                pos = (pos + step) & mask;
            while (pos >= high);
        }
    }
    if (pos != 0)
        return kCorrupt;
    for (uint32_t u = 0; u < size; ++u) {
        const uint32_t s = t[u].sym; // < nsym
        const uint32_t ns = next[s]++;
        const uint32_t nb = log - highbit(ns);
        t[u].nb = uint8_t(nb);
        t[u].base = uint16_t((ns << nb) - size);
    }
    return kOk;
}

// ---- Huffman --------------------------------------------------------------------
// The tree description at s[0, n): t.huf / t.huf_log, and the bytes it takes.
AQZ_ZINL uint32_t
huf_read_tree(const uint8_t* s, uint32_t n, Tables& t, uint32_t& used)
{
    if (n < 1)
        return kCorrupt;
    const uint32_t hb = s[0];
    uint32_t nw = 0;
    if (hb >= 128) { // direct: 4 bits per weight
        nw = hb - 127;
        const uint32_t bytes = (nw + 1) / 2;
        if (1 + bytes > n)
            return kCorrupt;
        for (uint32_t i = 0; i < nw; ++i) {
            const uint32_t b = s[1 + i / 2];
            t.weights[i] = uint8_t((i & 1u) ? (b & 15u) : (b >> 4));
        }
        used = 1 + bytes;
    } else { // FSE-compressed, two interleaved states
        if (hb == 0 || 1 + hb > n)
            return kCorrupt;
        uint32_t log = 0, hdr = 0;
        uint32_t e = fse_read_norm(s + 1, hb, 12, kWeightLog, t.norm, log, hdr);
        if (e != kOk)
            return e;
        e = fse_build(t.wt, t.norm, 13, log, t.next);
        if (e != kOk)
            return e;
        if (hdr >= hb)
            return kCorrupt;
        BitR r;
        if (!r.init(s + 1 + hdr, hb - hdr))
            return kCorrupt;
        uint32_t s1 = r.read(log), s2 = r.read(log);
        if (r.pos < 0)
            return kCorrupt;
        for (;;) {
            if (nw + 2 > 255)
                return kCorrupt;
            t.weights[nw++] = t.wt[s1].sym;
            s1 = t.wt[s1].base + r.read(t.wt[s1].nb);
            if (r.pos < 0) {
                t.weights[nw++] = t.wt[s2].sym;
                break;
            }
            if (nw + 2 > 255)
                return kCorrupt;
            t.weights[nw++] = t.wt[s2].sym;
            s2 = t.wt[s2].base + r.read(t.wt[s2].nb);
            if (r.pos < 0) {
                t.weights[nw++] = t.wt[s1].sym;
                break;
            }
        }
        used = 1 + hb;
    }
    if (nw == 0 || nw > 255)
        return kCorrupt;
    // the last weight completes the sum to a power of two
    uint32_t sum = 0;
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t w = t.weights[i];
        if (w > kHufLog)
            return kCorrupt;
        if (w)
            sum += 1u << (w - 1);
    }
    if (sum == 0)
        return kCorrupt;
    const uint32_t log = highbit(sum) + 1;
    if (log > kHufLog)
        return kCorrupt;
    const uint32_t left = (1u << log) - sum;
    if (left & (left - 1)) // left > 0 by the choice of log
        return kCorrupt;
    t.weights[nw++] = uint8_t(highbit(left) + 1);
    // cells of the table in order of weight, then of symbol
    for (uint32_t w = 0; w <= kHufLog + 1; ++w)
        t.rank[w] = 0;
    for (uint32_t i = 0; i < nw; ++i)
        t.rank[t.weights[i]] += 1;
    uint32_t start = 0;
    for (uint32_t w = 1; w <= kHufLog; ++w) {
        const uint32_t cnt = t.rank[w];
        t.rank[w] = start;
        start += cnt << (w - 1);
    }
    // start == 1 << log: sum + left
    for (uint32_t i = 0; i < nw; ++i) {
        const uint32_t w = t.weights[i];
        if (!w)
            continue;
        const uint32_t len = 1u << (w - 1);
        const uint16_t e = uint16_t(i | (log + 1 - w) << 8);
        const uint32_t at = t.rank[w];
        for (uint32_t k = 0; k < len; ++k)
            t.huf[at + k] = e;
        t.rank[w] = at + len;
    }
    t.huf_log = log;
    return kOk;
}

// One Huffman stream s[0, n) that must give exactly `count` literals.
AQZ_ZINL uint32_t
huf_decode_stream(const uint8_t* s, uint32_t n, const uint16_t* tab, uint32_t log, uint8_t* lit,
                  uint32_t count)
{
    BitR r;
    if (!r.init(s, n))
        return kCorrupt;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t e = tab[r.peek(log)]; // < 1 << log
        r.pos -= int32_t(e >> 8);
        if (r.pos < 0)
            return kCorrupt;
        lit[i] = uint8_t(e);
    }
    return r.pos == 0 ? kOk : kCorrupt;
}

// The streams of a Huffman literals section (filled by literals_section).
struct HufJob
{
    uint32_t ns;     // 1 or 4
    uint32_t src[4]; // start within the block's bytes
    uint32_t len[4];
    uint32_t dst[4]; // first literal
    uint32_t cnt[4];
};

// ---- frame ----------------------------------------------------------------------
struct FrameHeader
{
    uint32_t header_bytes;
    uint32_t checksum; // 4 bytes follow the last block
};

constexpr uint32_t kMagic = dec::kZstdMagic;

// The frame header of f[0, len) that must decode to n_dst bytes.
AQZ_ZINL uint32_t
parse_frame_header(const uint8_t* f, uint32_t len, uint64_t n_dst, FrameHeader& h)
{
    if (len < 4)
        return kBadHeader;
    const uint32_t magic = dec::rd32(f);
    if ((magic & 0xfffffff0u) == dec::kSkippableMagic)
        return kUnsupported; // a skippable frame
    if (magic != kMagic)
        return kBadHeader;
    if (len < 5)
        return kBadHeader;
    const uint32_t d = f[4];
    if (d & 0x08u)
        return kBadHeader; // reserved bit
    const uint32_t single = (d >> 5) & 1u, fcs_flag = d >> 6, did_flag = d & 3u;
    const uint32_t did_bytes = did_flag == 3 ? 4 : did_flag;
    const uint32_t fcs_bytes = fcs_flag == 0 ? single : 1u << fcs_flag;
    uint32_t pos = 5 + (single ? 0u : 1u);
    if (uint64_t(pos) + did_bytes + fcs_bytes > len)
        return kBadHeader;
    uint32_t did = 0;
    for (uint32_t k = 0; k < did_bytes; ++k)
        did |= uint32_t(f[pos + k]) << (8 * k);
    if (did != 0)
        return kUnsupported;
    pos += did_bytes;
    if (fcs_bytes) {
        uint64_t fcs = 0;
        for (uint32_t k = 0; k < fcs_bytes; ++k)
            fcs |= uint64_t(f[pos + k]) << (8 * k);
        if (fcs_bytes == 2)
            fcs += 256;
        if (fcs != n_dst)
            return kBadHeader;
        pos += fcs_bytes;
    }
    h.header_bytes = pos;
    h.checksum = (d & 0x04u) ? 4u : 0u;
    return kOk;
}

// What carries over from block to block of a frame.
struct FrameState
{
    uint32_t rep0, rep1, rep2;
};

// Literals of the block being decoded: where they come from.
struct Lits
{
    uint32_t kind; // 0 raw (source bytes at src), 1 RLE (byte), 2 the literal buffer
    uint32_t src;  // within the frame
    uint32_t byte;
    uint32_t n;
};

// The literals section at b[0, n) (the block's bytes, which start at boff in
// the frame): the literal source and the bytes the section takes.  Huffman literals are decoded into io's literal
// buffer by io.huf(...).  room: output bytes left; a block's literals all go
// to the output, so more of them than that is an error (and the literal
// buffer never holds more than the frame decodes to).
template<typename Io>
AQZ_ZINL uint32_t
literals_section(Io& io, const uint8_t* b, uint32_t boff, uint32_t n, uint32_t room, Tables& t,
                 Lits& L, uint32_t& used)
{
    if (n < 1)
        return kCorrupt;
    const uint32_t b0 = b[0], type = b0 & 3u, sf = (b0 >> 2) & 3u;
    if (type < 2) { // Raw, RLE
        uint32_t hdr, regen;
        if (sf == 0 || sf == 2) {
            hdr = 1;
            regen = b0 >> 3;
        } else if (sf == 1) {
            if (n < 2)
                return kCorrupt;
            hdr = 2;
            regen = (b0 >> 4) | uint32_t(b[1]) << 4;
        } else {
            if (n < 3)
                return kCorrupt;
            hdr = 3;
            regen = (b0 >> 4) | uint32_t(b[1]) << 4 | uint32_t(b[2]) << 12;
        }
        if (regen > kBlockMax || regen > room)
            return kCorrupt;
        L.n = regen;
        if (type == 0) {
            if (regen > n - hdr)
                return kCorrupt;
            L.kind = 0;
            L.src = boff + hdr;
            used = hdr + regen;
        } else {
            if (n - hdr < 1)
                return kCorrupt;
            L.kind = 1;
            L.byte = b[hdr];
            used = hdr + 1;
        }
        return kOk;
    }
    // Compressed (a tree description first), Treeless (the last tree)
    const uint32_t hdr = sf < 2 ? 3u : sf + 2u; // 3, 3, 4, 5
    const uint32_t bits = sf < 2 ? 10u : sf == 2 ? 14u : 18u;
    if (n < hdr)
        return kCorrupt;
    uint64_t v = 0;
    for (uint32_t k = 0; k < hdr; ++k)
        v |= uint64_t(b[k]) << (8 * k);
    v >>= 4;
    const uint32_t regen = uint32_t(v & ((1u << bits) - 1u));
    const uint32_t comp = uint32_t((v >> bits) & ((1u << bits) - 1u));
    if (regen > kBlockMax || regen > room || comp > n - hdr)
        return kCorrupt;
    uint32_t p = hdr, left = comp;
    if (type == 2) {
        uint32_t tree = 0;
        const uint32_t e = huf_read_tree(b + p, left, t, tree);
        if (e != kOk)
            return e;
        p += tree;
        left -= tree;
    } else if (t.huf_log == 0) {
        return kCorrupt; // nothing to repeat
    }
    HufJob j;
    j.ns = sf == 0 ? 1u : 4u;
    if (j.ns == 1) {
        j.src[0] = p;
        j.len[0] = left;
        j.dst[0] = 0;
        j.cnt[0] = regen;
    } else {
        if (left < 6)
            return kCorrupt;
        const uint32_t s1 = b[p] | uint32_t(b[p + 1]) << 8, s2 = b[p + 2] | uint32_t(b[p + 3]) << 8,
                       s3 = b[p + 4] | uint32_t(b[p + 5]) << 8;
        if (uint64_t(6) + s1 + s2 + s3 > left)
            return kCorrupt; // the jump table leaves the literals
        const uint32_t seg = (regen + 3) / 4;
        if (3 * seg > regen)
            return kCorrupt;
        j.src[0] = p + 6;
        j.len[0] = s1;
        j.src[1] = j.src[0] + s1;
        j.len[1] = s2;
        j.src[2] = j.src[1] + s2;
        j.len[2] = s3;
        j.src[3] = j.src[2] + s3;
        j.len[3] = left - 6 - s1 - s2 - s3;
        for (uint32_t k = 0; k < 4; ++k) {
            j.dst[k] = k * seg;
            j.cnt[k] = k < 3 ? seg : regen - 3 * seg;
        }
    }
    const uint32_t e = io.huf(b, j, t.huf, t.huf_log);
    if (e != kOk)
        return e;
    L.kind = 2;
    L.n = regen;
    used = hdr + comp;
    return kOk;
}

// One of the three sequence tables, by its mode; p moves past what it reads.
AQZ_ZINL uint32_t
seq_table(const uint8_t* b, uint32_t n, uint32_t& p, uint32_t mode, uint32_t which, Tables& t)
{
    FseEntry* tab = which == 0 ? t.ll : which == 1 ? t.of : t.ml;
    uint32_t& log = which == 0 ? t.ll_log : which == 1 ? t.of_log : t.ml_log;
    uint32_t& have = which == 0 ? t.have_ll : which == 1 ? t.have_of : t.have_ml;
    const uint32_t max_sym = which == 0 ? kLLMax : which == 1 ? kOFMax : kMLMax;
    const uint32_t max_log = which == 0 ? kLLLog : which == 1 ? kOFLog : kMLLog;
    if (mode == 3)
        return have ? kOk : kCorrupt;
    if (mode == 1) { // RLE: one symbol, no state bits
        if (p >= n)
            return kCorrupt;
        const uint32_t s = b[p++];
        if (s > max_sym)
            return kCorrupt;
        tab[0].sym = uint8_t(s);
        tab[0].nb = 0;
        tab[0].base = 0;
        log = 0;
        have = 1;
        return kOk;
    }
    uint32_t nsym, l;
    if (mode == 0) {
        nsym = which == 0 ? 36u : which == 1 ? 29u : 53u;
        l = which == 1 ? 5u : 6u;
        for (uint32_t s = 0; s < nsym; ++s)
            t.norm[s] = int16_t(which == 0 ? ll_default(s) : which == 1 ? of_default(s) : ml_default(s));
    } else {
        uint32_t used = 0;
        const uint32_t e = fse_read_norm(b + p, n - p, max_sym, max_log, t.norm, l, used);
        if (e != kOk)
            return e;
        if (used > n - p)
            return kCorrupt;
        p += used;
        nsym = max_sym + 1;
    }
    have = 0;
    const uint32_t e = fse_build(tab, t.norm, nsym, l, t.next);
    if (e != kOk)
        return e;
    log = l;
    have = 1;
    return kOk;
}

// A compressed block f[boff, boff + n): its bytes are appended at out
// position d (d moves); the output ends at n_dst.
//   io.huf(b, job, tab, log)     decode the Huffman streams (b + job.src[k])
//                                into io's literal buffer (cnt[k] literals at
//                                dst[k], all below kBlockMax); the status
//   io.copy_src(d, q, n)         out[d .. d+n) = f[q .. q+n)
//   io.copy_lit(d, i, n)         out[d .. d+n) = literal buffer[i .. i+n)
//   io.fill(d, v, n)             out[d .. d+n) = v
//   io.match(d, off, n)          out[d + i] = out[d - off + i % off], i < n
// Every call is made with its ranges already checked.
template<typename Io>
AQZ_ZINL void
put_literals(Io& io, const Lits& L, uint32_t d, uint32_t i, uint32_t n)
{
    if (!n)
        return;
    if (L.kind == 0)
        io.copy_src(d, L.src + i, n);
    else if (L.kind == 1)
        io.fill(d, L.byte, n);
    else
        io.copy_lit(d, i, n);
}

template<typename Io>
AQZ_ZINL uint32_t
compressed_block(Io& io, const uint8_t* f, uint32_t boff, uint32_t n, Tables& t, FrameState& fs,
                 uint32_t& d, uint32_t n_dst)
{
    Lits L{};
    uint32_t p = 0;
    const uint8_t* b = f + boff;
    uint32_t e = literals_section(io, b, boff, n, n_dst - d, t, L, p);
    if (e != kOk)
        return e;
    // sequences section header
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
    if (nseq == 0) {
        if (p != n)
            return kCorrupt;
        if (L.n > n_dst - d)
            return kCorrupt;
        put_literals(io, L, d, 0, L.n);
        d += L.n;
        return kOk;
    }
    if (p >= n)
        return kCorrupt;
    const uint32_t modes = b[p++];
    if (modes & 3u)
        return kCorrupt;
    e = seq_table(b, n, p, modes >> 6, 0, t);
    if (e == kOk)
        e = seq_table(b, n, p, (modes >> 4) & 3u, 1, t);
    if (e == kOk)
        e = seq_table(b, n, p, (modes >> 2) & 3u, 2, t);
    if (e != kOk)
        return e;
    BitR r;
    if (p >= n || !r.init(b + p, n - p))
        return kCorrupt;
    // states below 1 << log by construction: base + read(nb) < size
    uint32_t sl = r.read(t.ll_log), so = r.read(t.of_log), sm = r.read(t.ml_log);
    if (r.pos < 0)
        return kCorrupt;
    uint32_t li = 0; // literals taken
    for (uint32_t q = 0; q < nseq; ++q) {
        const FseEntry el = t.ll[sl], eo = t.of[so], em = t.ml[sm];
        const uint32_t ofc = eo.sym;
        if (ofc > kOFMax)
            return kCorrupt;
        uint32_t ov = (1u << ofc) + r.read(ofc);
        uint32_t mbase, mnb, lbase, lnb;
        ml_base(em.sym <= kMLMax ? em.sym : kMLMax, mbase, mnb);
        ll_base(el.sym <= kLLMax ? el.sym : kLLMax, lbase, lnb);
        const uint32_t ml = mbase + r.read(mnb);
        const uint32_t ll = lbase + r.read(lnb);
        if (q + 1 < nseq) {
            sl = el.base + r.read(el.nb);
            sm = em.base + r.read(em.nb);
            so = eo.base + r.read(eo.nb);
        }
        if (r.pos < 0)
            return kCorrupt;
        // the repeat offsets
        uint32_t off;
        if (ov > 3) {
            off = ov - 3;
            fs.rep2 = fs.rep1;
            fs.rep1 = fs.rep0;
            fs.rep0 = off;
        } else {
            const uint32_t idx = ov + (ll == 0 ? 1u : 0u); // 1..4
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
        if (ll > L.n - li || ll > n_dst - d)
            return kCorrupt;
        put_literals(io, L, d, li, ll);
        li += ll;
        d += ll;
        if (off == 0 || off > d || ml > n_dst - d)
            return kCorrupt;
        io.match(d, off, ml);
        d += ml;
    }
    if (r.pos != 0)
        return kCorrupt;
    const uint32_t rest = L.n - li;
    if (rest > n_dst - d)
        return kCorrupt;
    put_literals(io, L, d, li, rest);
    d += rest;
    return kOk;
}

// One zstd frame f[0, len) that must decode to exactly n_dst bytes (io's
// output).  t is scratch the caller owns (its contents do not matter).
template<typename Io>
AQZ_ZINL uint32_t
zstd_decode_frame(Io& io, const uint8_t* f, uint32_t len, uint32_t n_dst, Tables& t)
{
    FrameHeader h{};
    uint32_t e = parse_frame_header(f, len, n_dst, h);
    if (e != kOk)
        return e;
    t.huf_log = 0;
    t.have_ll = t.have_of = t.have_ml = 0;
    t.ll_log = t.of_log = t.ml_log = 0;
    FrameState fs{ 1, 4, 8 };
    uint32_t pos = h.header_bytes, d = 0;
    for (;;) {
        if (len - pos < 3)
            return kCorrupt; // no last block before the frame ends
        const uint32_t bh = f[pos] | uint32_t(f[pos + 1]) << 8 | uint32_t(f[pos + 2]) << 16;
        pos += 3;
        const uint32_t last = bh & 1u, type = (bh >> 1) & 3u, size = bh >> 3;
        if (type == 3 || size > kBlockMax)
            return kCorrupt;
        if (type == 1) { // RLE: one byte, `size` times
            if (len - pos < 1 || size > n_dst - d)
                return kCorrupt;
            if (size)
                io.fill(d, f[pos], size);
            d += size;
            pos += 1;
        } else {
            if (size > len - pos)
                return kCorrupt;
            if (type == 0) {
                if (size > n_dst - d)
                    return kCorrupt;
                if (size)
                    io.copy_src(d, pos, size);
                d += size;
            } else {
                e = compressed_block(io, f, pos, size, t, fs, d, n_dst);
                if (e != kOk)
                    return e;
            }
            pos += size;
        }
        if (last)
            break;
    }
    if (len - pos != h.checksum)
        return kCorrupt;
    return d == n_dst ? kOk : kCorrupt;
}

} // namespace zdec

} // namespace aqz
