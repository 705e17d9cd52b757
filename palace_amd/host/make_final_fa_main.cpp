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
#include "fast_exit.hpp"
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

[[noreturn]] void fault(const std::string &file, int64_t line, const std::string &reason)
{
    throw Failure(file + ": line " + std::to_string(line) + ": " + reason);
}

void open_text(palace_host::MappedText &t, const std::string &path)
{
    try { t.open(path); }
    catch (const std::exception &) { throw Failure("cannot open " + path); }
}

// strings -> ids: one name table over the strings themselves, each followed by a '+' so that the bytes `S+` are at once record S
// of the table's text and the token palace_path_resolve takes the name S from.  The id of a string is its first record.
std::vector<int32_t> ids_of(palace_ctx *ctx, const std::vector<fsv> &strings)
{
    std::string text;
    std::vector<palace_fasta_rec> recs;
    std::vector<int64_t> off{0};
    for (const fsv s : strings) {
        recs.push_back(palace_fasta_rec{static_cast<int64_t>(text.size()), static_cast<int64_t>(s.size()), 0, 0, 0, 0});
        text.append(s);
        text.push_back('+');
        off.push_back(static_cast<int64_t>(text.size()));
    }
    std::vector<int32_t> id(strings.size());
    if (strings.empty()) return id;
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const uint8_t *d_text = dev.upload(reinterpret_cast<const uint8_t *>(text.data()), text.size(), "the node names");
    const palace_fasta_rec *d_recs = dev.upload(recs.data(), recs.size(), "the node names' records");
    const int64_t *d_off = dev.upload(off.data(), off.size(), "the node names' offsets");
    int32_t *d_code = dev.array<int32_t>(strings.size(), "the node ids");
    palace_host::FastaNamesHandle names(ctx);
    HIP_OK(palace_fasta_names_create(ctx, d_text, d_recs, static_cast<int64_t>(recs.size()), nullptr, &names.h));
    HIP_OK(palace_path_resolve(ctx, names.h, d_text, d_off, static_cast<int64_t>(strings.size()), d_code));
    HIP_OK(palace_d2h(ctx, id.data(), d_code, id.size() * sizeof(int32_t)));
    for (int32_t &c : id) {
        if (c < 0 || (c & 3)) throw Failure("internal: a node name did not resolve to itself");
        c >>= 2;
    }
    return id;
}

void run(palace_ctx *ctx, const Args &a, palace_host::Trace &tr)
{
    palace_host::MappedText ptext, gtext, ftext;
    open_text(ptext, a.paths);
    open_text(gtext, a.graph);
    open_text(ftext, a.fasta);
    tr.lap("files read");
    const palace_host::FinalGraph g = palace_host::final_graph(gtext.data, gtext.size);
    if (g.fault.line) fault(a.graph, g.fault.line, g.fault.reason);
    const palace_host::FinalPaths pt = palace_host::final_paths(ptext.data, ptext.size);
    if (pt.fault.line) fault(a.paths, pt.fault.line, pt.fault.reason);
    const int64_t n_tok = static_cast<int64_t>(pt.tokens.size()), n_paths = static_cast<int64_t>(pt.paths());
    const size_t n_nodes = g.nodes.size();
    tr.lap("tokens split");

    // the assembly: text, index, names; two records of one name are a fault
    DeviceScope as(ctx, palace_host::no_room_does_not_fit);
    palace_host::FastaNamesHandle names(ctx);
    const int64_t fn = static_cast<int64_t>(ftext.size);
    const uint8_t *d_text = as.upload(ftext.bytes(), ftext.size, "the FASTA is read on the device and has no other path: it");
    const palace_host::FastaIndex ix = palace_host::index_fasta(ctx, as, d_text, fn, "the FASTA's index");
    if (ix.st.error) fault(a.fasta, ix.st.bad_line, palace_host::fasta_fault_text(ix.st.error));
    palace_fasta_rec *const d_recs = ix.d_recs;
    {
        const std::vector<uint8_t> dup = palace_host::hash_names(ctx, as, d_text, d_recs, ix.st.n_records, names);
        for (size_t k = 0; k < dup.size(); k++)
            if (dup[k]) {                                                    // (rare: the record comes to the host only to be named)
                palace_fasta_rec r;
                HIP_OK(palace_d2h(ctx, &r, d_recs + k, sizeof r));
                int64_t line = 1;
                for (int64_t i = 0; i < r.name_off; i++) line += ftext.data[i] == '\n';
                fault(a.fasta, line, "sequence name '" + std::string(ftext.data + r.name_off, static_cast<size_t>(r.name_len)) + "' appears a second time");
            }
    }
    tr.lap("FASTA indexed, names hashed");

    // ids of the JUNC nodes, the tokens and the tokens' bases
    std::vector<fsv> strings;
    for (size_t k = 0; k < n_nodes; k++) strings.push_back(g.nodes.at(k));
    for (int64_t t = 0; t < n_tok; t++) strings.push_back(pt.tokens.at(static_cast<size_t>(t)));
    for (int64_t t = 0; t < n_tok; t++) strings.push_back(palace_host::final_base(pt.tokens.at(static_cast<size_t>(t))));
    const std::vector<int32_t> id = ids_of(ctx, strings);
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
    std::vector<int32_t> code(static_cast<size_t>(n_tok));
    {
        std::string q;
        std::vector<int64_t> q_off{0};
        for (int64_t t = 0; t < n_tok; t++) {
            q += palace_host::final_query(pt.tokens.at(static_cast<size_t>(t)));
            q_off.push_back(static_cast<int64_t>(q.size()));
        }
        const uint8_t *d_q = dev.upload(reinterpret_cast<const uint8_t *>(q.data()), q.size(), "the tokens");
        const int64_t *d_q_off = dev.upload(q_off.data(), q_off.size(), "the tokens' offsets");
        int32_t *d_code = dev.array<int32_t>(static_cast<size_t>(n_tok), "the tokens' records");
        HIP_OK(palace_path_resolve(ctx, names.h, d_q, d_q_off, n_tok, d_code));
        if (n_tok) HIP_OK(palace_d2h(ctx, code.data(), d_code, code.size() * sizeof(int32_t)));
    }
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
    std::string hdr;
    std::vector<int64_t> hdr_off{0}, path_out{0};
    int64_t count = 0;
    for (int64_t p = 0; p < n_paths; p++) {
        int64_t bytes = 0;
        if (len[static_cast<size_t>(p)] > 0) {                              // a path without sequence is not written and takes no number
            const size_t before = hdr.size();
            hdr += a.prefix + "_phage_" + std::to_string(++count) + (out_cycle[static_cast<size_t>(p)] ? "_cycle" : "_linear");
            bytes = static_cast<int64_t>(hdr.size() - before) + len[static_cast<size_t>(p)] + 3;
        }
        hdr_off.push_back(static_cast<int64_t>(hdr.size()));
        path_out.push_back(path_out.back() + bytes);
    }
    const int64_t total = path_out.back();
    const uint8_t *d_hdr = dev.upload(reinterpret_cast<const uint8_t *>(hdr.data()), hdr.size(), "the headers");
    const int64_t *d_hdr_off = dev.upload(hdr_off.data(), hdr_off.size(), "the headers' offsets");
    const int64_t *d_path_out = dev.upload(path_out.data(), path_out.size(), "the paths' places");
    tr.lap("lengths and headers");

    // windows of the output text: window w is computed and copied back while window w - 1 goes to the file
    const std::string tmp = a.out + ".tmp";
    std::FILE *out = std::fopen(tmp.c_str(), "wb");
    if (!out) throw Failure("cannot write " + tmp);
    palace_host::FileGuard closer{out, tmp.c_str()};
    if (total) {
        palace_host::WindowWriter windows(ctx, dev, "PALACE_FINALFA_WINDOW", total);
        windows.write(total, out, tmp, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_final_fasta_write(ctx, d_text, d_recs, d_out_code, d_cum, d_out_off, n_paths, d_hdr, d_hdr_off, d_path_out, kSepByte, lo, hi, d_win));
        });
    }
    closer.release();
    if (std::fclose(out) != 0 || std::rename(tmp.c_str(), a.out.c_str()) != 0) {
        std::remove(tmp.c_str());
        throw Failure("cannot write " + a.out);
    }
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
    palace_host::FastExit fast_exit = palace_host::fast_exit_begin();   // from here on this is the worker process (fast_exit.hpp)
    const int device = palace_host::pick_device();                       // PALACE_DEVICE (device_pick.hpp): before anything touches HIP
    palace_host::Trace tr("make_final_fa");
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(device, &ctx) != PALACE_OK) {
        std::fprintf(stderr, "make_final_fa: no GPU device to work on (%s); there is no CPU path\n", palace_last_error());
        return 1;
    }
    tr.lap("device up");
    try {
        run(ctx, a, tr);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "make_final_fa: %s\n", e.what());
        return 1;
    }
    fast_exit.done(0);          // the output is complete and renamed: the caller goes on, the teardown happens behind it
}
