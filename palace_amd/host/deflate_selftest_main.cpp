// The member encoder of palace_bgzf_deflate (csrc/deflate_enc.hpp) on a CPU: the kernel's phases run thread by thread, in thread
// order, over a file cut into members of 0xff00 bytes -- the same tokens, codes and bits the workgroup produces, without a device.
//     deflate_selftest <text file> <out.gz>      writes the members and the EOF member; what inflates them is the caller's (zlib)
//     deflate_selftest batch <pieces> <lengths> <misalignment> <members out> <member lengths out>
//                                                one member per piece of the concatenated pieces, each read at that misalignment
//     deflate_selftest codes <histograms> <codes out>
//                                                enc_rank + enc_build_code on histograms of any alphabet and bit limit
// tests/test_host_deflate_enc.py and tests/test_host_deflate_enc_edges.py drive it.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../csrc/deflate_enc.hpp"

using namespace palace;

static uint32_t encode_member(EncShared &s, const uint8_t *text, int n, std::vector<uint32_t> &slot)
{
    slot.assign(kEncSlot / 4, 0xeeeeeeeeu);
    if (n == 0) {
        for (int t = 0; t < kEncThreads; t++) enc_write_empty(t, slot.data());
        return 28;
    }
    s.n = n; s.mis = static_cast<int>(reinterpret_cast<uintptr_t>(text) & 3);
    s.chunk = (n + kEncThreads - 1) / kEncThreads;
    s.crc = static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), text, static_cast<uInt>(n)));
    std::memcpy(reinterpret_cast<uint8_t *>(s.text) + s.mis, text, static_cast<size_t>(n));
    auto all = [&](auto phase) { for (int t = 0; t < kEncThreads; t++) phase(t); };
    all([&](int t) { enc_phase_clear(s, t); });
    all([&](int t) { enc_phase_freq(s, t); });
    all([&](int t) { enc_phase_sort(s, t); });
    all([&](int t) { enc_phase_codes(s, t); });
    all([&](int t) { enc_phase_cl_freq(s, t); });
    all([&](int t) { enc_phase_cl_code(s, t); });
    all([&](int t) { enc_phase_bits(s, t); });
    enc_scan_serial(s);
    // in the reverse thread order: what is written must not depend on who comes first
    for (int t = kEncThreads - 1; t >= 0; t--) enc_phase_write(s, t, slot.data());
    all([&](int t) { enc_phase_merge(s, t, slot.data()); });
    return s.member_len;
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
// lies at misalignment `mis`.  The exact size guards this driver's own reads of the piece (crc32, the copy into s.text) under a
// sanitizer, nothing more: the encoder reads s.text, inside EncShared, where a read past n is not an overflow any sanitizer sees --
// what holds enc_walk to n is the token list the tests compare.
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
    auto s = std::make_unique<EncShared>();
    std::vector<uint32_t> slot;
    size_t at = 0, stored = 0;
    for (const long n : lengths) {
        if (at + static_cast<size_t>(n) > pieces.size()) { std::fprintf(stderr, "%s is shorter than its lengths\n", pieces_path); return 1; }
        std::unique_ptr<uint8_t[]> piece(new uint8_t[static_cast<size_t>(mis + n)]);     // (operator new aligns to 16 bytes)
        if ((reinterpret_cast<uintptr_t>(piece.get()) & 3) != 0) { std::fprintf(stderr, "unaligned allocation\n"); return 1; }
        if (n) std::memcpy(piece.get() + mis, pieces.data() + at, static_cast<size_t>(n));
        const uint32_t m = encode_member(*s, piece.get() + mis, static_cast<int>(n), slot);
        stored += n && s->stored;
        if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
        std::fprintf(out_len, "%u\n", m);
        at += static_cast<size_t>(n);
    }
    if (std::fclose(out) != 0 || std::fclose(out_len) != 0) return 1;
    std::printf("%zu members, %zu stored\n", lengths.size(), stored);
    return 0;
}

// One histogram per line: <symbols> <bit limit> <frequency of symbol 0> <of symbol 1> ...  The code of each, ranked and built as the
// phases do it (enc_phase_sort, enc_phase_codes), leaves as a line of lengths and a line of codes (bit-reversed, as the writer keeps them).
static int codes(const char *path, const char *out_path)
{
    std::vector<uint8_t> text;
    if (!read_file(path, text)) return 1;
    FILE *out = std::fopen(out_path, "w");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", out_path); return 1; }
    text.push_back(0);
    char *p = reinterpret_cast<char *>(text.data());
    for (;;) {
        char *end;
        const long n_sym = std::strtol(p, &end, 10);
        if (end == p) break;
        p = end;
        const long max_bits = std::strtol(p, &end, 10);
        if (end == p || n_sym < 1 || n_sym > 288 || max_bits < 1 || max_bits > 15) { std::fprintf(stderr, "bad histogram head\n"); return 1; }
        p = end;
        uint32_t freq[288], key[288];
        uint16_t sorted[288], code[288];
        uint8_t len[288];
        for (long t = 0; t < n_sym; t++) {
            const unsigned long f = std::strtoul(p, &end, 10);
            if (end == p) { std::fprintf(stderr, "histogram of fewer than %ld entries\n", n_sym); return 1; }
            freq[t] = static_cast<uint32_t>(f); key[t] = 0; sorted[t] = 0; code[t] = 0; len[t] = 0;
            p = end;
        }
        for (long t = 0; t < n_sym; t++) enc_rank(freq, static_cast<int>(n_sym), static_cast<int>(t), key, sorted);
        enc_build_code(freq, static_cast<int>(n_sym), static_cast<int>(max_bits), key, sorted, len, code);
        for (long t = 0; t < n_sym; t++) std::fprintf(out, "%d%c", len[t], t + 1 < n_sym ? ' ' : '\n');
        for (long t = 0; t < n_sym; t++) std::fprintf(out, "%d%c", code[t], t + 1 < n_sym ? ' ' : '\n');
    }
    return std::fclose(out) == 0 ? 0 : 1;
}

int main(int argc, char **argv)
{
    if (argc == 7 && std::strcmp(argv[1], "batch") == 0) return batch(argv[2], argv[3], std::atoi(argv[4]), argv[5], argv[6]);
    if (argc == 4 && std::strcmp(argv[1], "codes") == 0) return codes(argv[2], argv[3]);
    if (argc != 3) {
        std::fprintf(stderr, "Usage: %s <text file> <out.gz>\n       %s batch <pieces> <lengths> <misalignment> <members out> <member lengths out>\n"
                             "       %s codes <histograms> <codes out>\n", argv[0], argv[0], argv[0]);
        return 1;
    }
    FILE *in = std::fopen(argv[1], "rb");
    if (!in) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    std::vector<uint8_t> text(3);                                         // (members start at every misalignment)
    uint8_t buf[65536];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, in)) > 0;) text.insert(text.end(), buf, buf + k);
    std::fclose(in);
    FILE *out = std::fopen(argv[2], "wb");
    if (!out) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    auto s = std::make_unique<EncShared>();
    std::vector<uint32_t> slot;
    const size_t n = text.size() - 3;
    size_t members = 0, stored = 0;
    for (size_t at = 0; at < n || members == 0; at += kEncMaxText, members++) {
        const int len = static_cast<int>(n - at < static_cast<size_t>(kEncMaxText) ? n - at : kEncMaxText);
        const uint32_t m = encode_member(*s, text.data() + 3 + at, len, slot);
        stored += len && s->stored;
        if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
        if (len == 0) break;
    }
    if (n) {
        const uint32_t m = encode_member(*s, nullptr, 0, slot);
        if (std::fwrite(slot.data(), 1, m, out) != m) return 1;
    }
    if (std::fclose(out) != 0) return 1;
    std::printf("%zu members, %zu stored\n", members, stored);
    return 0;
}
