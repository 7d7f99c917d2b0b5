// zstddec_sanitize.cpp -- the device zstd decoder's parse (csrc/aqz_zstddec.hh:
// frame header, block walk, literals and sequences sections, Huffman and FSE
// table builds, bit readers, sequence decode, repeat offsets, every bound; and
// csrc/aqz_lz4dec.hh for the blosc1 container) run on the host under ASan +
// UBSan with serial byte movers, over a corpus file written by
// tests/test_zstddec_cpu.py.
//
// Corpus: as tests/sanitize/lz4dec_sanitize.cpp reads it ("AQZC", u32 n; per
// record u32 name_len, name, i32 expected status (-1: any), u64 chunk_bytes,
// u32 frame_len, frame, u32 expected_len, expected bytes).  Every frame is
// decoded from a heap copy of exactly its size into heap buffers of exactly
// the chunk / block / literal size, so that any read or write past an end is
// a sanitizer report.
#include "aqz_zstddec.hh"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace aqz;

namespace {

struct HostIo
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

uint32_t
decode_zstd(const uint8_t* f, uint32_t len, uint8_t* out, uint32_t n_dst)
{
    auto t = std::make_unique<zdec::Tables>();
    HostIo io{ f, out, nullptr };
    return zdec::zstd_decode_frame(io, f, len, n_dst, *t);
}

// The whole frame, as the device kernels do it: the status is the largest
// any block reports.
uint32_t
decode_frame(const uint8_t* f, uint64_t len, uint64_t chunk_bytes, uint8_t* out)
{
    if (len == 0) {
        std::memset(out, 0, chunk_bytes);
        return dec::kSkipped;
    }
    if (f[0] != 2) // not a blosc1 frame: a plain zstd frame
        return decode_zstd(f, uint32_t(len), out, uint32_t(chunk_bytes));
    dec::FrameInfo h{};
    const uint32_t st = dec::parse_header(f, len, chunk_bytes, h, dec::kCodecZstd);
    if (st != dec::kOk)
        return st;
    if (h.memcpyed) {
        std::memcpy(out, f + 16, h.nbytes);
        return dec::kOk;
    }
    uint32_t worst = dec::kOk;
    for (uint32_t j = 0; j < h.nblocks; ++j) {
        const dec::BlockInfo bi = dec::block_info(h, j);
        std::unique_ptr<uint8_t[]> tmp(new uint8_t[bi.bsize]);
        uint32_t pos = 0;
        uint32_t e = dec::block_start(f, h, j, pos);
        for (uint32_t s = 0; s < bi.ns && e == dec::kOk; ++s) {
            uint32_t src = 0, csz = 0;
            e = dec::next_stream(f, h, pos, src, csz);
            if (e != dec::kOk)
                break;
            uint8_t* o = tmp.get() + size_t(s) * bi.slen;
            if (csz == bi.slen)
                std::memcpy(o, f + src, bi.slen);
            else
                e = decode_zstd(f + src, csz, o, bi.slen);
        }
        if (e != dec::kOk) {
            worst = e > worst ? e : worst;
            continue;
        }
        uint8_t* o = out + size_t(j) * h.blocksize;
        for (uint32_t x = 0; x < bi.bsize; ++x)
            o[x] = dec::unshuffled_byte(tmp.get(), bi.bsize, h.typesize, h.mode, x);
    }
    return worst;
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
        std::fprintf(stderr, "usage: %s corpus\n", argv[0]);
        return 2;
    }
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
        std::unique_ptr<uint8_t[]> out(new uint8_t[chunk_bytes]);
        std::memset(out.get(), 0xA5, chunk_bytes);
        const uint32_t st = decode_frame(frame.get(), frame_len, chunk_bytes, out.get());
        std::printf("%s %u\n", name.c_str(), st);
        if (expect >= 0 && st != uint32_t(expect)) {
            std::printf("FAIL %s: status %u, expected %d\n", name.c_str(), st, expect);
            ++failures;
        }
        if (st <= dec::kSkipped && expect >= 0 && expect <= int32_t(dec::kSkipped)) {
            if (exp_len != chunk_bytes ||
                (exp_len && std::memcmp(out.get(), want.data(), exp_len) != 0)) {
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
