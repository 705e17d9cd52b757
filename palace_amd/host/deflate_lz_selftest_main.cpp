// The member encoder of palace_bgzf_deflate_lz (csrc/deflate_lz.hpp over csrc/deflate_enc.hpp) on a CPU: the kernel's phases run thread
// by thread -- the rounds of the head table with every thread's look before any thread's entry, as the barriers order them on the
// device -- so that the same tokens, codes and bits leave as the workgroup's, without a device.
//     deflate_lz_selftest <file> <out.gz>        the file cut into members of 0xff00 bytes and the EOF member; zlib inflates them (the caller)
//     deflate_lz_selftest batch <pieces> <lengths> <misalignment> <members out> <member lengths out>
//                                                one member per piece of the concatenated pieces, each read at that misalignment
// tests/test_host_deflate_lz.py drives it.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../csrc/deflate_lz.hpp"

using namespace palace;

static uint32_t encode_member(LzShared &s, const uint8_t *text, int n, std::vector<uint32_t> &slot)
{
    slot.assign(kEncSlot / 4, 0xeeeeeeeeu);
    if (n == 0) {
        for (int t = 0; t < kEncThreads; t++) enc_write_empty(t, slot.data());
        return 28;
    }
    EncShared &e = s.e;
    e.n = n; e.mis = static_cast<int>(reinterpret_cast<uintptr_t>(text) & 3);
    e.chunk = (n + kEncThreads - 1) / kEncThreads;
    e.crc = static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), text, static_cast<uInt>(n)));
    std::memcpy(reinterpret_cast<uint8_t *>(e.text) + e.mis, text, static_cast<size_t>(n));
    std::unique_ptr<uint16_t[]> dist(new uint16_t[static_cast<size_t>(n)]);            // exactly n entries: a walk past n is an overflow the sanitizer sees
    auto all = [&](auto phase) { for (int t = 0; t < kEncThreads; t++) phase(t); };
    all([&](int t) { enc_phase_clear(e, t); });
    all([&](int t) { lz_phase_clear(s, t); });
    for (int r = 0; r < lz_rounds(e); r++) {
        for (int t = kEncThreads - 1; t >= 0; t--) lz_phase_look(s, t, r, dist.get());
        for (int t = kEncThreads - 1; t >= 0; t--) lz_phase_enter(s, t, r);            // (in the reverse order: a max does not care)
    }
    const LzWalk walk{dist.get()};
    all([&](int t) { enc_phase_freq(e, t, walk); });
    all([&](int t) { enc_phase_sort(e, t); });
    all([&](int t) { enc_phase_codes(e, t); });
    all([&](int t) { enc_phase_cl_freq(e, t); });
    all([&](int t) { enc_phase_cl_code(e, t); });
    all([&](int t) { enc_phase_bits(e, t, walk); });
    enc_scan_serial(e);
    for (int t = kEncThreads - 1; t >= 0; t--) enc_phase_write(e, t, slot.data(), walk);
    all([&](int t) { enc_phase_merge(e, t, slot.data()); });
    return e.member_len;
}

static bool read_file(const char *path, std::vector<uint8_t> &data)
{
    FILE *in = std::fopen(path, "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", path); return false; }
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, in)) > 0;) data.insert(data.end(), buf, buf + k);
    std::fclose(in);
    return true;
}

// Pieces given by their lengths, one member each: piece k is copied to an allocation of exactly mis + n bytes, so that its first byte
// lies at misalignment `mis`.
static int batch(const char *pieces_path, const char *lengths_path, int mis, const char *members_path, const char *member_lengths_path)
{
    std::vector<uint8_t> pieces, lengths_text;
    if (mis < 0 || mis > 3) { std::fprintf(stderr, "misalignment %d: 0 .. 3\n", mis); return 1; }
    if (!read_file(pieces_path, pieces) || !read_file(lengths_path, lengths_text)) return 1;
    lengths_text.push_back(0);
    std::vector<long> lengths;
    for (char *p = reinterpret_cast<char *>(lengths_text.data());;) {
        char *end;
        const long v = std::strtol(p, &end, 10);
        if (end == p) break;
        if (v < 0 || v > kEncMaxText) { std::fprintf(stderr, "piece of %ld bytes: 0 .. %d\n", v, kEncMaxText); return 1; }
        lengths.push_back(v);
        p = end;
    }
    FILE *out = std::fopen(members_path, "wb"), *out_len = std::fopen(member_lengths_path, "w");
    if (!out || !out_len) { std::fprintf(stderr, "cannot open %s or %s\n", members_path, member_lengths_path); return 1; }
    auto s = std::make_unique<LzShared>();
    std::vector<uint32_t> slot;
    size_t at = 0, stored = 0;
    for (const long n : lengths) {
        if (at + static_cast<size_t>(n) > pieces.size()) { std::fprintf(stderr, "%s is shorter than its lengths\n", pieces_path); return 1; }
        std::unique_ptr<uint8_t[]> piece(new uint8_t[static_cast<size_t>(mis + n)]);     // (operator new aligns to 16 bytes)
        if ((reinterpret_cast<uintptr_t>(piece.get()) & 3) != 0) { std::fprintf(stderr, "unaligned allocation\n"); return 1; }
        if (n) std::memcpy(piece.get() + mis, pieces.data() + at, static_cast<size_t>(n));
        const uint32_t m = encode_member(*s, piece.get() + mis, static_cast<int>(n), slot);
        stored += n && s->e.stored;
        if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
        std::fprintf(out_len, "%u\n", m);
        at += static_cast<size_t>(n);
    }
    if (std::fclose(out) != 0 || std::fclose(out_len) != 0) return 1;
    std::printf("%zu members, %zu stored\n", lengths.size(), stored);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && std::strcmp(argv[1], "batch") == 0) return batch(argv[2], argv[3], std::atoi(argv[4]), argv[5], argv[6]);
    if (argc != 3) {
        std::fprintf(stderr, "Usage: %s <file> <out.gz>\n       %s batch <pieces> <lengths> <misalignment> <members out> <member lengths out>\n", argv[0], argv[0]);
        return 1;
    }
    std::vector<uint8_t> text(3);                                         // (members start at every misalignment)
    if (!read_file(argv[1], text)) return 1;
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    auto s = std::make_unique<LzShared>();
    std::vector<uint32_t> slot;
    const size_t n = text.size() - 3;
    size_t members = 0, stored = 0;
    for (size_t at = 0; at < n; at += kEncMaxText, members++) {
        const int len = static_cast<int>(n - at < static_cast<size_t>(kEncMaxText) ? n - at : kEncMaxText);
        const uint32_t m = encode_member(*s, text.data() + 3 + at, len, slot);
        stored += s->e.stored;
        if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
    }
    const uint32_t m = encode_member(*s, nullptr, 0, slot);
    if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
    if (std::fclose(out) != 0) return 1;
    std::printf("%zu members, %zu stored\n", members, stored);
    return 0;
}
