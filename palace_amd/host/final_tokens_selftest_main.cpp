// final_tokens.hpp on its own (tests/test_host_final_fa_rules.py; also built with the host sanitizers).
//   final_tokens_selftest graph <file>: per arc `A <source, hex> <source's length> <destination, hex> <destination's length>`
//   final_tokens_selftest paths <file>: per path `L <1-based line> <tokens>` and per token `T <token, hex> <length> <base, hex>
//                                       <what is looked up in the assembly, hex>`
// A faulty file gives the one line `F <1-based line> <reason>` instead.
#include <cstdio>
#include <fstream>
#include <iterator>
#include <string>

#include "final_tokens.hpp"

using palace_host::fsv;

static void hex(fsv s)
{
    if (s.empty()) std::fputc('-', stdout);
    for (const char c : s) std::printf("%02x", static_cast<unsigned char>(c));
}

int main(int argc, char **argv)
{
    const std::string mode = argc == 3 ? argv[1] : "";
    if (mode != "graph" && mode != "paths") { std::fprintf(stderr, "usage: final_tokens_selftest graph|paths <file>\n"); return 2; }
    std::ifstream f(argv[2], std::ios::binary);
    if (!f) { std::fprintf(stderr, "final_tokens_selftest: cannot open %s\n", argv[2]); return 1; }
    const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (mode == "graph") {
        const palace_host::FinalGraph g = palace_host::final_graph(text.data(), text.size());
        if (g.fault.line) { std::printf("F %lld %s\n", static_cast<long long>(g.fault.line), g.fault.reason); return 0; }
        for (size_t k = 0; k + 1 < g.nodes.size(); k += 2) {
            std::fputs("A ", stdout);
            hex(g.nodes.at(k));
            std::printf(" %lld ", static_cast<long long>(g.len[k]));
            hex(g.nodes.at(k + 1));
            std::printf(" %lld\n", static_cast<long long>(g.len[k + 1]));
        }
        return 0;
    }
    const palace_host::FinalPaths p = palace_host::final_paths(text.data(), text.size());
    if (p.fault.line) { std::printf("F %lld %s\n", static_cast<long long>(p.fault.line), p.fault.reason); return 0; }
    for (size_t k = 0; k < p.paths(); k++) {
        std::printf("L %lld %lld\n", static_cast<long long>(p.line_no[k]), static_cast<long long>(p.line_tok[k + 1] - p.line_tok[k]));
        for (int64_t t = p.line_tok[k]; t < p.line_tok[k + 1]; t++) {
            const fsv tok = p.tokens.at(static_cast<size_t>(t));
            std::fputs("T ", stdout);
            hex(tok);
            std::printf(" %lld ", static_cast<long long>(p.len[static_cast<size_t>(t)]));
            hex(palace_host::final_base(tok));
            std::fputc(' ', stdout);
            hex(palace_host::final_query(tok));
            std::fputc('\n', stdout);
        }
    }
    return 0;
}
