// zstdpar_sanitize.cpp -- the block-parallel zstd decode (csrc/aqz_zstdpar.hh:
// index, block entropy decode, placement, execute) run on the host under
// ASan + UBSan with serial byte movers, over a corpus file written by
// tests/test_zstdpar_cpu.py, and compared record by record with the serial
// parse (zdec::zstd_decode_frame): the same status, and the same bytes when
// the status is OK.
//
// Corpus: as tests/sanitize/zstddec_sanitize.cpp reads it.  Every buffer has
// exactly its declared size -- the frame, the output, the block table
// (zpar::block_capacity, or argv[2] blocks), the literal area (n_dst bytes)
// and the records (zpar::record_capacity) -- so that any read or write past
// an end is a sanitizer report.  The phases run in the kernels' order: every
// block's entropy decode, then placement, then every copy, then the match
// chain; copies and matches are not interleaved.
//
// Output per record: "<name> <status> <taken|fallback|other>": taken = the
// parallel phases decoded (or refused) the frame, fallback = more blocks than
// the table holds (the serial parse's result stands), other = not a plain
// zstd frame (blosc1 container, zero length: not this path's).
#include "aqz_zstdpar.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace aqz;

namespace {

// movers of the serial parse (as zstddec_sanitize.cpp)
struct SerialIo
{
    const uint8_t* src;
    uint8_t* out;
    std::unique_ptr<uint8_t[]> lit;
    uint32_t huf(const uint8_t* f, const zdec::HufJob& j, const uint16_t* tab, uint32_t log)
    {
        const uint32_t total = j.dst[j.ns - 1] + j.cnt[j.ns - 1];
        lit.reset(new uint8_t[total]);
        uint32_t worst = dec::kOk;
        for (uint32_t k = 0; k < j.ns; ++k) {
            const uint32_t e =
              zdec::huf_decode_stream(f + j.src[k], j.len[k], tab, log, lit.get() + j.dst[k], j.cnt[k]);
            worst = e > worst ? e : worst;
        }
        return worst;
    }
    void copy_src(uint32_t d, uint32_t q, uint32_t n) { std::memcpy(out + d, src + q, n); }
    void copy_lit(uint32_t d, uint32_t i, uint32_t n) { std::memcpy(out + d, lit.get() + i, n); }
    void fill(uint32_t d, uint32_t v, uint32_t n) { std::memset(out + d, int(v), n); }
    void match(uint32_t d, uint32_t off, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i)
            out[d + i] = out[d - off + i % off];
    }
};

// movers of the entropy phase: one block's literal area, the frame's records
struct EntropyIo
{
    uint8_t* lit;
    zpar::Record* rec;
    uint32_t huf(const uint8_t* f, const zdec::HufJob& j, const uint16_t* tab, uint32_t log)
    {
        uint32_t worst = dec::kOk;
        for (uint32_t k = 0; k < j.ns; ++k) {
            const uint32_t e =
              zdec::huf_decode_stream(f + j.src[k], j.len[k], tab, log, lit + j.dst[k], j.cnt[k]);
            worst = e > worst ? e : worst;
        }
        return worst;
    }
    void record(uint32_t i, uint32_t ll, uint32_t ml, uint32_t ov)
    {
        rec[i] = zpar::Record{ ll, ml, ov };
    }
};

// movers of the execute phase
struct ExecIo
{
    const uint8_t* src;
    uint8_t* out;
    const uint8_t* lit; // the frame's literal area
    void copy_src(uint32_t d, uint32_t q, uint32_t n) { std::memcpy(out + d, src + q, n); }
    void copy_lit(uint32_t d, uint32_t i, uint32_t n) { std::memcpy(out + d, lit + i, n); }
    void fill(uint32_t d, uint32_t v, uint32_t n) { std::memset(out + d, int(v), n); }
    void match(uint32_t d, uint32_t off, uint32_t n)
    {
        for (uint32_t i = 0; i < n; ++i)
            out[d + i] = out[d - off + i % off];
    }
};

uint32_t
decode_serial(const uint8_t* f, uint32_t len, uint8_t* out, uint32_t n_dst)
{
    auto t = std::make_unique<zdec::Tables>();
    SerialIo io{ f, out, nullptr };
    return zdec::zstd_decode_frame(io, f, len, n_dst, *t);
}

uint32_t
decode_parallel(const uint8_t* f, uint32_t len, uint8_t* out, uint32_t n_dst, uint32_t cap,
                bool& taken)
{
    std::unique_ptr<zpar::Block[]> tab(new zpar::Block[cap]);
    std::unique_ptr<uint8_t[]> lit(new uint8_t[n_dst]);
    std::unique_ptr<zpar::Record[]> rec(new zpar::Record[zpar::record_capacity(n_dst)]);
    uint32_t nb = 0, nseq = 0;
    uint32_t e = zpar::par_index(f, len, n_dst, tab.get(), cap, nb, nseq, taken);
    if (!taken || e != dec::kOk)
        return e;
    auto t = std::make_unique<zdec::Tables>();
    uint32_t worst = dec::kOk;
    for (uint32_t j = 0; j < nb; ++j) { // every block on its own, as on the device
        if (tab[j].type != 2)
            continue;
        EntropyIo io{ lit.get() + tab[j].lit_off, rec.get() };
        uint32_t regen = 0;
        e = zpar::par_entropy(io, f, tab.get(), j, n_dst, *t, regen);
        tab[j].regen = e == dec::kOk ? regen : 0u;
        worst = e > worst ? e : worst;
    }
    if (worst != dec::kOk)
        return worst;
    e = zpar::par_place(tab.get(), nb, n_dst);
    if (e != dec::kOk)
        return e;
    ExecIo io{ f, out, lit.get() };
    for (uint32_t j = 0; j < nb; ++j)
        zpar::par_copy_block(io, f, tab[j], rec.get());
    return zpar::par_matches(io, rec.get(), nseq);
}

bool
rd(FILE* fp, void* p, size_t n)
{
    return n == 0 || std::fread(p, 1, n, fp) == n;
}

} // namespace

int
main(int argc, char** argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s corpus [block table capacity]\n", argv[0]);
        return 2;
    }
    const long fixed_cap = argc > 2 ? std::atol(argv[2]) : 0;
    FILE* fp = std::fopen(argv[1], "rb");
    if (!fp)
        return 2;
    char magic[4];
    uint32_t n = 0;
    if (!rd(fp, magic, 4) || std::memcmp(magic, "AQZC", 4) != 0 || !rd(fp, &n, 4))
        return 2;
    int failures = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t name_len = 0, frame_len = 0, exp_len = 0;
        int32_t expect = -1;
        uint64_t chunk_bytes = 0;
        if (!rd(fp, &name_len, 4))
            return 2;
        std::string name(name_len, '\0');
        if (!rd(fp, name.data(), name_len) || !rd(fp, &expect, 4) || !rd(fp, &chunk_bytes, 8) ||
            !rd(fp, &frame_len, 4))
            return 2;
        std::unique_ptr<uint8_t[]> frame(new uint8_t[frame_len]);
        if (!rd(fp, frame.get(), frame_len) || !rd(fp, &exp_len, 4))
            return 2;
        std::vector<uint8_t> want(exp_len);
        if (!rd(fp, want.data(), exp_len))
            return 2;
        // the kernels' test of "a plain zstd frame of this run"
        const bool plain = frame_len != 0 &&
                           dec::frame_family(frame.get(), frame_len) == dec::kFamilyZstd &&
                           (dec::rd32(frame.get()) == dec::kZstdMagic ||
                            (dec::rd32(frame.get()) & 0xfffffff0u) == dec::kSkippableMagic);
        if (!plain) {
            std::printf("%s %d other\n", name.c_str(), expect);
            continue;
        }
        const uint32_t n_dst = uint32_t(chunk_bytes);
        std::unique_ptr<uint8_t[]> ser(new uint8_t[n_dst]), par(new uint8_t[n_dst]);
        std::memset(ser.get(), 0xA5, n_dst);
        std::memset(par.get(), 0x5A, n_dst);
        const uint32_t st_ser = decode_serial(frame.get(), frame_len, ser.get(), n_dst);
        bool taken = false;
        const uint32_t cap = fixed_cap > 0 ? uint32_t(fixed_cap) : zpar::block_capacity(n_dst);
        uint32_t st = decode_parallel(frame.get(), frame_len, par.get(), n_dst, cap, taken);
        const uint8_t* got = par.get();
        if (!taken) { // the serial kernel's frame
            st = st_ser;
            got = ser.get();
        }
        std::printf("%s %u %s\n", name.c_str(), st, taken ? "taken" : "fallback");
        if (st != st_ser) {
            std::printf("FAIL %s: status %u, the serial parse's %u\n", name.c_str(), st, st_ser);
            ++failures;
        }
        if (expect >= 0 && st != uint32_t(expect)) {
            std::printf("FAIL %s: status %u, expected %d\n", name.c_str(), st, expect);
            ++failures;
        }
        if (st == dec::kOk && st_ser == dec::kOk && n_dst &&
            std::memcmp(got, ser.get(), n_dst) != 0) {
            std::printf("FAIL %s: bytes differ from the serial parse's\n", name.c_str());
            ++failures;
        }
        if (st == dec::kOk && expect == int32_t(dec::kOk)) {
            if (exp_len != chunk_bytes || (exp_len && std::memcmp(got, want.data(), exp_len) != 0)) {
                std::printf("FAIL %s: decoded bytes differ\n", name.c_str());
                ++failures;
            }
        }
    }
    std::fclose(fp);
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("clean: %u records\n", n);
    return 0;
}
