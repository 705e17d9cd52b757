// make_final_fa <final.txt> <filtered_graph.txt> <assembly_graph.fasta> <final.fasta> <prefix> [--trim_threshold N]
// [--min_cycle_length N]: the reference's share/palace/scripts/make_final_fa.py (call site palace:877-882) with its command line
// and its stderr, the cycle test of every path, the FASTA's index and the output text on the device (csrc/final_fasta.hip,
// csrc/path_fasta.hip; the rules: DESIGN.md 8).  The host reads the three files, splits the two small ones into tokens
// (final_tokens.hpp), turns strings into ids through a name table on the device, writes the headers, the warnings, the totals and
// the file; it decides no cycle and produces no sequence byte.  There is no path around the device.
// PALACE_FINALFA_WINDOW: bytes of output text per window (default 256 MiB), as PALACE_PATHFA_WINDOW of make_fa_from_path.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "final_tokens.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "trace.hpp"

namespace {

using palace_host::DeviceScope;
using palace_host::Failure;
using palace_host::fsv;
using palace_host::line_fault;

constexpr int64_t kSepLen = 50;
constexpr int32_t kSepByte = 'N';

struct Args {
    std::string paths, graph, fasta, out, prefix;
    int64_t trim_threshold = 300, min_cycle_length = 10000;
};

bool parse_int(const char *s, int64_t *out)
{
    if (!*s) return false;
    char *end = nullptr;
    errno = 0;
    const long long v = std::strtoll(s, &end, 10);
    if (errno || *end || s[0] == ' ') return false;
    *out = v;
    return true;
}

// the two options in their full spelling, `--name N` or `--name=N`, anywhere among the five positionals
bool parse_args(int argc, char **argv, Args *a)
{
    std::vector<std::string> pos;
    for (int k = 1; k < argc; k++) {
        const std::string s = argv[k];
        int64_t *dst = nullptr;
        const char *value = nullptr;
        for (const char *name : {"--trim_threshold", "--min_cycle_length"}) {
            const size_t n = std::strlen(name);
            int64_t *d = name[2] == 't' ? &a->trim_threshold : &a->min_cycle_length;
            if (s == name) { if (k + 1 >= argc) return false; dst = d; value = argv[++k]; }
            else if (s.compare(0, n + 1, std::string(name) + "=") == 0) { dst = d; value = argv[k] + n + 1; }
        }
        if (dst) { if (!parse_int(value, dst)) return false; continue; }
        if (s.size() > 1 && s[0] == '-' && (s[1] < '0' || s[1] > '9')) return false;          // an option this program does not have
        pos.push_back(s);
    }
    if (pos.size() != 5) return false;
    a->paths = pos[0]; a->graph = pos[1]; a->fasta = pos[2]; a->out = pos[3]; a->prefix = pos[4];
    return true;
}

void run(palace_ctx *ctx, const Args &a, palace_host::Trace &tr)
{
    palace_host::MappedText ptext, gtext;
    palace_host::open_text(ptext, a.paths);
    palace_host::open_text(gtext, a.graph);
    palace_host::Assembly as(ctx, a.fasta);
    tr.lap("files read");
    const palace_host::FinalGraph g = palace_host::final_graph(gtext.data, gtext.size);
    if (g.fault.line) line_fault(a.graph, g.fault.line, g.fault.reason);
    const palace_host::FinalPaths pt = palace_host::final_paths(ptext.data, ptext.size);
    if (pt.fault.line) line_fault(a.paths, pt.fault.line, pt.fault.reason);
    const int64_t n_tok = static_cast<int64_t>(pt.tokens.size()), n_paths = static_cast<int64_t>(pt.paths());
    const size_t n_nodes = g.nodes.size();
    tr.lap("tokens split");

    // the assembly: text, index, names; two records of one name are a fault
    as.load(tr, [&](size_t, const palace_fasta_rec &r, const char *text) {
        line_fault(a.fasta, palace_host::line_of(text, r.name_off), "sequence name '" + std::string(text + r.name_off, static_cast<size_t>(r.name_len)) + "' appears a second time");
    });
    const uint8_t *const d_text = as.d_text;
    palace_fasta_rec *const d_recs = as.d_recs;

    // ids of the JUNC nodes, the tokens and the tokens' bases
    std::vector<fsv> strings;
    for (size_t k = 0; k < n_nodes; k++) strings.push_back(g.nodes.at(k));
    for (int64_t t = 0; t < n_tok; t++) strings.push_back(pt.tokens.at(static_cast<size_t>(t)));
    for (int64_t t = 0; t < n_tok; t++) strings.push_back(palace_host::final_base(pt.tokens.at(static_cast<size_t>(t))));
    const std::vector<int32_t> id = palace_host::ids_of(ctx, strings);
    std::vector<uint64_t> arcs(n_nodes / 2);
    for (size_t k = 0; k < arcs.size(); k++) arcs[k] = (static_cast<uint64_t>(static_cast<uint32_t>(id[2 * k])) << 32) | static_cast<uint32_t>(id[2 * k + 1]);
    tr.lap("ids");

    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const int64_t *d_path_off = dev.upload(pt.line_tok.data(), pt.line_tok.size(), "the paths' tokens");
    std::vector<int32_t> first(static_cast<size_t>(n_paths)), last(static_cast<size_t>(n_paths));
    {
        const int32_t *d_node = dev.upload(id.data() + n_nodes, static_cast<size_t>(n_tok), "the tokens' ids");
        const int32_t *d_base = dev.upload(id.data() + n_nodes + n_tok, static_cast<size_t>(n_tok), "the bases' ids");
        const int64_t *d_len = dev.upload(pt.len.data(), pt.len.size(), "the tokens' lengths");
        uint64_t *d_arcs = dev.upload(arcs.data(), arcs.size(), "the arcs");
        const size_t sb = palace_sort_u64_scratch_bytes(static_cast<int64_t>(arcs.size()));
        uint32_t *d_perm = dev.array<uint32_t>(arcs.size(), "the arcs' order");
        void *d_scratch = dev.alloc(sb, "the sort's scratch");
        HIP_OK(palace_sort_u64(ctx, d_arcs, d_perm, static_cast<int64_t>(arcs.size()), 64, d_scratch, sb));
        int32_t *d_first = dev.array<int32_t>(static_cast<size_t>(n_paths), "the kept intervals"), *d_last = dev.array<int32_t>(static_cast<size_t>(n_paths), "the kept intervals");
        HIP_OK(palace_cycle_trim(ctx, d_node, d_base, d_len, n_tok, d_path_off, n_paths, d_arcs, static_cast<int64_t>(arcs.size()), a.trim_threshold,
                                 a.min_cycle_length, d_first, d_last));
        if (n_paths) {
            HIP_OK(palace_d2h(ctx, first.data(), d_first, first.size() * sizeof(int32_t)));
            HIP_OK(palace_d2h(ctx, last.data(), d_last, last.size() * sizeof(int32_t)));
        }
    }
    tr.lap("cycles decided");

    // the tokens in the assembly
    std::string q;
    std::vector<int64_t> q_off{0};
    for (int64_t t = 0; t < n_tok; t++) {
        q += palace_host::final_query(pt.tokens.at(static_cast<size_t>(t)));
        q_off.push_back(static_cast<int64_t>(q.size()));
    }
    const std::vector<int32_t> code = palace_host::resolve(ctx, dev, as.names.h, q, q_off, palace_host::kTokensWhat, true).code;
    // the output's paths: the cycles, cut, in file order, then the others, whole; a token whose name is no record is warned about
    std::vector<int32_t> out_code;
    std::vector<int64_t> out_off{0};
    std::vector<uint8_t> out_cycle;
    int64_t n_cycle = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int64_t p = 0; p < n_paths; p++) {
            const bool cyc = first[static_cast<size_t>(p)] >= 0;
            if (cyc != (pass == 0)) continue;
            n_cycle += cyc;
            const int64_t t0 = pt.line_tok[static_cast<size_t>(p)] + (cyc ? first[static_cast<size_t>(p)] : 0);
            const int64_t t1 = cyc ? pt.line_tok[static_cast<size_t>(p)] + last[static_cast<size_t>(p)] + 1 : pt.line_tok[static_cast<size_t>(p) + 1];
            for (int64_t t = t0; t < t1; t++) {
                int32_t c = code[static_cast<size_t>(t)];
                if (c < 0 || (c & PALACE_PATH_SECOND_TRY)) {
                    const std::string q = palace_host::final_query(pt.tokens.at(static_cast<size_t>(t)));
                    std::fprintf(stderr, "Warning: Node '%s' not found in %s\n", q.substr(0, q.size() - 1).c_str(), a.fasta.c_str());
                    c = PALACE_PATH_NOT_FOUND;
                }
                out_code.push_back(c);
            }
            out_off.push_back(static_cast<int64_t>(out_code.size()));
            out_cycle.push_back(cyc ? 1 : 0);
        }
    tr.lap("tokens resolved");

    const int64_t n_out_tok = static_cast<int64_t>(out_code.size());
    const int32_t *d_out_code = dev.upload(out_code.data(), out_code.size(), "the output's tokens");
    const int64_t *d_out_off = dev.upload(out_off.data(), out_off.size(), "the output's paths");
    int64_t *d_cum = dev.array<int64_t>(static_cast<size_t>(n_out_tok + 1), "the tokens' places");
    int64_t *d_len = dev.array<int64_t>(static_cast<size_t>(n_paths), "the paths' lengths");
    HIP_OK(palace_final_fasta_lengths(ctx, d_recs, d_out_code, n_out_tok, d_out_off, n_paths, kSepLen, d_cum, d_len));
    std::vector<int64_t> len(static_cast<size_t>(n_paths));
    if (n_paths) HIP_OK(palace_d2h(ctx, len.data(), d_len, len.size() * sizeof(int64_t)));
    palace_host::PathsText plan;
    int64_t count = 0;
    for (int64_t p = 0; p < n_paths; p++) {
        if (len[static_cast<size_t>(p)] > 0)                                // a path without sequence is not written and takes no number
            plan.add(a.prefix + "_phage_" + std::to_string(++count) + (out_cycle[static_cast<size_t>(p)] ? "_cycle" : "_linear"), len[static_cast<size_t>(p)]);
        else plan.skip();
    }
    const palace_host::PathsText::OnDevice pd = plan.upload(dev);
    tr.lap("lengths and headers");

    // windows of the output text: window w is computed and copied back while window w - 1 goes to the file
    palace_host::PendingOutputs outputs;
    std::FILE *out = outputs.open(a.out);
    if (pd.total) {
        palace_host::WindowWriter windows(ctx, dev, "PALACE_FINALFA_WINDOW", pd.total);
        windows.write(pd.total, out, a.out + ".tmp", [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_final_fasta_write(ctx, d_text, d_recs, d_out_code, d_cum, d_out_off, n_paths, pd.d_hdr, pd.d_hdr_off, pd.d_path_out, kSepByte, lo, hi, d_win));
        });
    }
    if (!outputs.commit()) throw Failure("cannot write " + a.out);
    tr.lap("output written");
    std::fprintf(stderr, "Total circular paths found: %lld\nTotal linear paths found: %lld\nFasta successfully written to: %s\n\n",
                 static_cast<long long>(n_cycle), static_cast<long long>(n_paths - n_cycle), a.out.c_str());
}

}  // namespace

int main(int argc, char **argv)
{
    Args a;
    if (!parse_args(argc, argv, &a)) {
        std::fputs("usage: make_final_fa [--trim_threshold N] [--min_cycle_length N] path_file graph_file edge_fasta out_fasta prefix\n", stderr);
        return 2;
    }
    return palace_host::device_tool("make_final_fa", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, a, tr); });
}
