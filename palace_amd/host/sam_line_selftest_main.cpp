// csrc/sam_line.hpp and host/sam_header.hpp on their own, on a CPU (tests/test_host_sam_rules.py; also built under ASan + UBSan):
//   sam_line_selftest <in.sam> <mask>
// prints `H <code>` and nothing else for a header sam_header.hpp refuses; otherwise one line per line behind the header:
//   R <hex of the record, block_size word included>     D (the mask drops it)     E <PALACE_SAM_E* code>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>
#include <unordered_map>
#include <vector>

#include "../csrc/sam_line.hpp"
#include "sam_header.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "Usage: sam_line_selftest <in.sam> <mask>\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "sam_line_selftest: cannot open %s\n", argv[1]); return 2; }
    const std::vector<uint8_t> text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const uint32_t mask = static_cast<uint32_t>(std::strtoul(argv[2], nullptr, 0));
    const uint8_t *t = text.data();
    const int64_t n = static_cast<int64_t>(text.size());
    const palace_host::SamHeader h = palace_host::parse_sam_header(t, text.size());
    if (h.code) { std::printf("H %d\n", h.code); return 0; }
    std::unordered_map<std::string, int32_t> tid;
    for (size_t k = 0; k < h.name.size(); k++) tid[h.name[k]] = static_cast<int32_t>(k);
    auto tid_of = [&](const uint8_t *p, int64_t len) {
        const auto it = tid.find(std::string(reinterpret_cast<const char *>(p), static_cast<size_t>(len)));
        return it == tid.end() ? -1 : it->second;
    };
    std::vector<uint8_t> rec;
    for (int64_t b = static_cast<int64_t>(h.text_bytes); b < n;) {
        int64_t e = b;
        while (e < n && t[e] != '\n') e++;
        if (e == b) std::printf("E %d\n", PALACE_SAM_EEMPTY);
        else if (t[b] == '@') std::printf("E %d\n", PALACE_SAM_EAT);
        else {
            const palace::SamLine s = palace::sam_line(t, b, e, mask, tid_of, nullptr, 0);
            if (s.code) std::printf("E %d\n", s.code);
            else if (s.size == 0) std::printf("D\n");
            else {
                rec.assign(static_cast<size_t>(s.size), 0xAA);               // exactly the record's bytes: a store past them is the sanitizer's
                palace::sam_line(t, b, e, mask, tid_of, rec.data(), 0);
                std::fputs("R ", stdout);
                for (uint8_t v : rec) std::printf("%02x", v);
                std::fputc('\n', stdout);
            }
        }
        b = e + 1;
    }
    return 0;
}
