// The sort key and the .bai interval of csrc/bam_record.hpp on their own (tests/test_host_bam_index_rules.py), as built and under
// the host sanitizers:   bam_index_selftest <records> <n_ref>
// <records>: raw BAM alignment records one behind the other (block_size word first), walked with walk_step.  Prints per record
// `sort key (or "bad") <TAB> beg <TAB> end <TAB> bin (-1: a .bai cannot hold the interval)`.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <vector>

#include "../csrc/bam_record.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "Usage: %s <records> <n_ref>\n", argv[0]); return 1; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    const std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const int32_t n_ref = static_cast<int32_t>(std::atol(argv[2]));
    const int64_t total = static_cast<int64_t>(d.size());
    int64_t p = 0, next = 0;
    while (palace::walk_step(d.data(), p, total, total, &next) == 1) {
        const int64_t s = p + 4;
        const palace::BaiSpan sp = palace::bai_span(d.data(), s);
        if (palace::sort_key_ok(d.data(), s, n_ref)) std::printf("%llu", static_cast<unsigned long long>(palace::sort_key(d.data(), s, n_ref)));
        else std::printf("bad");
        std::printf("\t%lld\t%lld\t%d\n", static_cast<long long>(sp.beg), static_cast<long long>(sp.end), sp.ok ? static_cast<int>(palace::reg2bin(sp.beg, sp.end)) : -1);
        p = next;
    }
    if (p != total) { std::fprintf(stderr, "malformed record at offset %lld\n", static_cast<long long>(p)); return 2; }
    return 0;
}
