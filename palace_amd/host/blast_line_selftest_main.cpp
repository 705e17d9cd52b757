// csrc/blast_line.hpp on a CPU (tests/test_host_blast_line.py, tests/test_host_filter_result_rules.py), as built and under the host
// sanitizers; nothing of the device is linked.
//   blast_line_selftest lines <file>    every line of the file (cut at LF, a last line without LF is a line), each copied into an
//                                       allocation of exactly its length: `L <identity digits> <decimals> <length>` or `E <code>`
//   blast_line_selftest cuts <ratio>    the seven cuts the executable makes of `ratio * 100`, one per line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/blast_line.hpp"

int main(int argc, char **argv)
{
    if (argc == 3 && std::strcmp(argv[1], "cuts") == 0) {
        int64_t cut[palace::kBlastCuts];
        palace::blast_identity_cuts(std::strtod(argv[2], nullptr) * 100.0, cut);
        for (const int64_t c : cut) std::printf("%lld\n", static_cast<long long>(c));
        return 0;
    }
    if (argc != 3 || std::strcmp(argv[1], "lines") != 0) {
        std::fputs("usage: blast_line_selftest lines <file> | cuts <ratio>\n", stderr);
        return 2;
    }
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    std::string text;
    char buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, k);
    std::fclose(f);
    for (size_t a = 0; a < text.size();) {
        const size_t lf = text.find('\n', a), e = lf == std::string::npos ? text.size() : lf;
        const std::vector<uint8_t> line(text.begin() + static_cast<std::ptrdiff_t>(a), text.begin() + static_cast<std::ptrdiff_t>(e));   // (exactly the line: a read past it is the sanitizer's)
        const palace::BlastLine l = palace::blast_line_parse(line.data(), static_cast<int64_t>(line.size()));
        if (l.error) std::printf("E %d\n", l.error);
        else std::printf("L %lld %d %lld\n", static_cast<long long>(l.ident), l.decimals, static_cast<long long>(l.length));
        a = e + 1;
    }
    return 0;
}
