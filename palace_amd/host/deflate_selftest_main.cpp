// The member encoder of palace_bgzf_deflate (csrc/deflate_enc.hpp) on a CPU: the kernel's phases run thread by thread, in thread
// order, over a file cut into members of 0xff00 bytes -- the same tokens, codes and bits the workgroup produces, without a device.
//     deflate_selftest <text file> <out.gz>      writes the members and the EOF member; what inflates them is the caller's (zlib)
// tests/test_host_deflate_enc.py drives it.
#include <zlib.h>

#include <cstdio>
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

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "Usage: %s <text file> <out.gz>\n", argv[0]); return 1; }
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
