// path_tokens.hpp on its own (tests/test_host_path_tokens.py; also built with the host sanitizers): prints, for every line of
// <paths file> that gives a record, `L <0-based line index> <tokens>` and per token `T <as split, hex> <cleaned, hex>` ('-' for
// no bytes).
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "path_tokens.hpp"

static void hex(const std::string &s, int64_t a, int64_t b)
{
    if (a == b) std::fputc('-', stdout);
    for (int64_t i = a; i < b; i++) std::printf("%02x", static_cast<unsigned char>(s[static_cast<size_t>(i)]));
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: path_tokens_selftest <paths file>\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "path_tokens_selftest: cannot open %s\n", argv[1]); return 1; }
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const palace_host::PathTokens t = palace_host::split_paths(text.data(), text.size());
    for (size_t k = 0; k < t.lines(); k++) {
        std::printf("L %lld %lld\n", static_cast<long long>(t.line_index[k]), static_cast<long long>(t.line_tok[k + 1] - t.line_tok[k]));
        for (int64_t i = t.line_tok[k]; i < t.line_tok[k + 1]; i++) {
            std::fputs("T ", stdout);
            hex(t.raw, t.raw_off[static_cast<size_t>(i)], t.raw_off[static_cast<size_t>(i) + 1]);
            std::fputc(' ', stdout);
            hex(t.clean, t.clean_off[static_cast<size_t>(i)], t.clean_off[static_cast<size_t>(i) + 1]);
            std::fputc('\n', stdout);
        }
    }
    return 0;
}
