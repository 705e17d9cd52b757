// corrected_dup [--contig-depth <table>] <out_dir> <prefix> <cycle_file> <final_all_file> <final.txt> <final.fasta> <edge_fasta>
// <cycle_nodup.txt> <bam> <before_cut> <min_len>: the reference's share/palace/scripts/corrected_dup.py (call site palace:864-875)
// with its command line.  It writes <out_dir>/<final.txt>, the paths make_final_fa turns into the result, and -- empty, as the
// script leaves it -- <out_dir>/<cycle_nodup.txt>; arguments 2 and 6 are taken and unused, as there.  The rules and the declared
// deviations: DESIGN.md 8.
// The host reads <edge_fasta>.fai, the two path files and <before_cut>, splits them into tokens, does the list surgery of one path and
// the double arithmetic (corrected_dup_rules.hpp) and writes the text.  The device resolves every name (a name table and
// palace_path_resolve), reads the BAM (bam_stream_device.hpp) and reduces it to a depth sum and a covered count per contig
// (palace_depth_per_contig), and decides what is quadratic or worse: borders, tandem candidates, the similarity relation, the
// base-set test (csrc/path_dedup.hip).  With --contig-depth the table `bamdepth --per-contig` printed (name TAB sum TAB covered)
// stands in for the BAM pass and argument 9 is not opened.  There is no path around the device and no host BAM reader.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "bam_stream_device.hpp"
#include "corrected_dup_rules.hpp"
#include "depth_host.hpp"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "fasta_device.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "trace.hpp"

namespace {

using palace_host::DeviceScope;
using palace_host::Failure;
using palace_host::line_fault;
namespace cdup = palace_host::cdup;
using cdup::Path;
using sv = std::string_view;

struct Args {
    std::string out_dir, cycles, finals, out_name, fasta, nodup_name, bam, before_cut, depth_table;
    int64_t min_len = 0;
};

bool parse_args(int argc, char **argv, Args *a)
{
    int k = 1;
    if (argc > 2 && std::strcmp(argv[1], "--contig-depth") == 0) { a->depth_table = argv[2]; k = 3; }
    if (argc - k != 11) return false;
    char **p = argv + k;
    a->out_dir = p[0]; a->cycles = p[2]; a->finals = p[3]; a->out_name = p[4]; a->fasta = p[6]; a->nodup_name = p[7]; a->bam = p[8]; a->before_cut = p[9];
    char *end = nullptr;
    errno = 0;
    const long long v = std::strtoll(p[10], &end, 10);
    if (errno || !*p[10] || *end) return false;
    a->min_len = v;
    return true;
}

// the smallest faulty line of a file
struct Fault {
    int64_t line = 0;
    std::string reason;
    void at(int64_t l, const std::string &r) { if (!line || l < line) { line = l; reason = r; } }
};

// the lines of a text (without their LF; a text that ends in LF has no line behind it)
std::vector<sv> lines_of(const palace_host::MappedText &t)
{
    std::vector<sv> out;
    const sv text(t.data ? t.data : "", t.size);
    for (size_t at = 0; at < text.size();) {
        const size_t e = std::min(text.find('\n', at), text.size());
        out.push_back(text.substr(at, e - at));
        at = e + 1;
    }
    return out;
}

bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }
sv strip(sv s)
{
    while (!s.empty() && is_space(s.front())) s.remove_prefix(1);
    while (!s.empty() && is_space(s.back())) s.remove_suffix(1);
    return s;
}
std::vector<sv> words_of(sv line)
{
    std::vector<sv> out;
    for (size_t at = 0; at < line.size();) {
        while (at < line.size() && is_space(line[at])) at++;
        size_t e = at;
        while (e < line.size() && !is_space(line[e])) e++;
        if (e > at) out.push_back(line.substr(at, e - at));
        at = e;
    }
    return out;
}

// Every word of the three files as (file, line, text); its token once the names are resolved.
struct Words {
    std::vector<sv> text;
    std::vector<int64_t> line;
    std::vector<int> file;
    size_t add(int f, int64_t l, sv w) { text.push_back(w); line.push_back(l); file.push_back(f); return text.size() - 1; }
};
struct Span { size_t first, count; };                               // words [first, first + count)

struct Flat {
    std::vector<int32_t> tok;
    std::vector<int64_t> off{0};
    explicit Flat(const std::vector<Path> &paths)
    {
        for (const Path &p : paths) { tok.insert(tok.end(), p.begin(), p.end()); off.push_back(static_cast<int64_t>(tok.size())); }
    }
    int64_t n_paths() const { return static_cast<int64_t>(off.size()) - 1; }
};

// the four questions of corrected_dup_rules.hpp's decide(), answered by csrc/path_dedup.hip
struct OnDevice {
    palace_ctx *ctx;
    const std::vector<int64_t> &fai_len;

    std::vector<int32_t> borders(const std::vector<Path> &paths)
    {
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const Flat f(paths);
        const int32_t *d_tok = dev.upload(f.tok.data(), f.tok.size(), "the cycles' tokens");
        const int64_t *d_off = dev.upload(f.off.data(), f.off.size(), "the cycles' lines");
        int32_t *d_border = dev.array<int32_t>(paths.size(), "the cycles' borders");
        HIP_OK(palace_path_borders(ctx, d_tok, d_off, f.n_paths(), d_border));
        std::vector<int32_t> border(paths.size());
        if (!paths.empty()) HIP_OK(palace_d2h(ctx, border.data(), d_border, border.size() * sizeof(int32_t)));
        return border;
    }
    void tandems(const std::vector<Path> &paths, std::vector<cdup::Candidate> *cand, std::vector<int64_t> *cand_off)
    {
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const Flat f(paths);
        const int32_t *d_tok = dev.upload(f.tok.data(), f.tok.size(), "the cycles' tokens");
        const int64_t *d_off = dev.upload(f.off.data(), f.off.size(), "the cycles' lines");
        int64_t *d_cand_off = dev.array<int64_t>(f.off.size(), "the candidates' places");
        int64_t n_cand = 0;
        HIP_OK(palace_path_tandems(ctx, d_tok, d_off, f.n_paths(), d_cand_off, nullptr, 0, &n_cand));
        int32_t *d_cand = dev.array<int32_t>(3 * static_cast<size_t>(n_cand), "the tandem candidates");
        HIP_OK(palace_path_tandems(ctx, d_tok, d_off, f.n_paths(), d_cand_off, d_cand, n_cand, &n_cand));
        cand->assign(static_cast<size_t>(n_cand), cdup::Candidate{});
        cand_off->assign(f.off.size(), 0);
        if (n_cand) HIP_OK(palace_d2h(ctx, cand->data(), d_cand, cand->size() * sizeof(cdup::Candidate)));
        if (!paths.empty()) HIP_OK(palace_d2h(ctx, cand_off->data(), d_cand_off, cand_off->size() * sizeof(int64_t)));
    }
    // the relation's bytes: pair (i, j) at bits 2 (k & 3) of byte k >> 2, k = i * n + j
    std::vector<uint8_t> relation(const std::vector<Path> &paths)
    {
        if (paths.size() >= (1u << 15)) throw Failure("more than 32767 paths to compare");
        const Flat f(paths);
        std::vector<int64_t> len;
        for (const int32_t t : f.tok) len.push_back(fai_len[static_cast<size_t>(cdup::base_of(t))]);
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const int64_t *d_len = dev.upload(len.data(), len.size(), "the tokens' lengths");
        const int64_t *d_off = dev.upload(f.off.data(), f.off.size(), "the paths' tokens");
        const size_t nb = palace_paths_length_relation_bytes(f.n_paths());
        uint8_t *d_rel = dev.array<uint8_t>(nb, "the paths' relation");
        HIP_OK(palace_paths_length_relation(ctx, d_len, static_cast<int64_t>(len.size()), d_off, f.n_paths(), d_rel));
        std::vector<uint8_t> rel(nb);
        if (nb) HIP_OK(palace_d2h(ctx, rel.data(), d_rel, nb));
        return rel;
    }
    std::vector<uint8_t> base_set_in(const std::vector<Path> &paths, size_t n_cycles)
    {
        const Flat f(paths);
        std::vector<int32_t> base;
        for (const int32_t t : f.tok) base.push_back(cdup::base_of(t));
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const int32_t *d_base = dev.upload(base.data(), base.size(), "the tokens' bases");
        const int64_t *d_off = dev.upload(f.off.data(), f.off.size(), "the paths' tokens");
        uint8_t *d_in = dev.array<uint8_t>(paths.size(), "the base-set verdicts");
        HIP_OK(palace_paths_base_set_in(ctx, d_base, static_cast<int64_t>(base.size()), d_off, f.n_paths(), static_cast<int64_t>(n_cycles), 64, d_in));
        std::vector<uint8_t> in(paths.size());
        if (!paths.empty()) HIP_OK(palace_d2h(ctx, in.data(), d_in, in.size()));
        return in;
    }
};

void run(palace_ctx *ctx, const Args &a, palace_host::Trace &tr)
{
    const std::string fai_path = a.fasta + ".fai";
    palace_host::MappedText fai_text, cycle_text, final_text, cut_text, table_text;
    palace_host::open_text(fai_text, fai_path);
    palace_host::open_text(cycle_text, a.cycles);
    palace_host::open_text(final_text, a.finals);
    palace_host::open_text(cut_text, a.before_cut);
    if (!a.depth_table.empty()) palace_host::open_text(table_text, a.depth_table);
    tr.lap("files read");

    // the index: names and lengths
    std::vector<sv> fai_name;
    std::vector<int64_t> fai_len;
    {
        int64_t l = 0;
        for (const sv row : lines_of(fai_text)) {
            l++;
            const size_t t1 = row.find('\t'), t2 = t1 == sv::npos ? sv::npos : std::min(row.find('\t', t1 + 1), row.size());
            int64_t v = 0;
            bool ok = t1 != sv::npos && t1 > 0 && t2 > t1 + 1;
            for (size_t k = t1 + 1; ok && k < t2; k++) { ok = row[k] >= '0' && row[k] <= '9' && v < (1ll << 40); v = v * 10 + (row[k] - '0'); }
            if (!ok || v > 0xffffffffll) line_fault(fai_path, l, "not a name and a length below 2^32");
            fai_name.push_back(row.substr(0, t1));
            fai_len.push_back(v);
        }
    }
    const size_t n_fai = fai_name.size();

    // the words of the three files; a fault of a word's shape is kept until the names are known: the smallest faulty line is reported
    const std::string *file_name[3] = {&a.before_cut, &a.cycles, &a.finals};
    Fault fault[3];
    Words words;
    auto add_words = [&](int f, int64_t l, sv text) {
        const Span s{words.text.size(), 0};
        size_t n = 0;
        for (const sv w : words_of(text)) {
            const char *why = cdup::token_fault(w);
            if (*why) fault[f].at(l, "'" + std::string(w) + "' " + why);
            words.add(f, l, w);
            n++;
        }
        return Span{s.first, n};
    };
    std::vector<std::pair<Span, Span>> cut_rows;
    {
        int64_t l = 0;
        for (const sv row : lines_of(cut_text)) {
            l++;
            const sv s = strip(row);
            const size_t colon = s.find(':');
            if (colon == sv::npos || s.find(':', colon + 1) != sv::npos) { fault[0].at(l, "not exactly one ':'"); continue; }
            if (colon == 0) continue;                                        // (an empty key is no entry)
            const Span key = add_words(0, l, s.substr(0, colon)), value = add_words(0, l, s.substr(colon + 1));
            cut_rows.emplace_back(key, value);
        }
    }
    std::vector<Span> cycle_rows, final_rows;
    {
        int64_t l = 0;
        for (const sv row : lines_of(cycle_text)) {
            const Span s = add_words(1, ++l, row);
            if (!s.count) fault[1].at(l, "a blank line");
            cycle_rows.push_back(s);
        }
        l = 0;
        for (const sv row : lines_of(final_text)) {
            const Span s = add_words(2, ++l, row);
            if (s.count) final_rows.push_back(s);
        }
    }
    tr.lap("tokens split");

    // the depth's source: the BAM through the device loader, or the table
    std::vector<std::string> depth_name;
    std::vector<uint64_t> depth_sum, depth_cov;
    if (a.depth_table.empty()) {
        palace_host::DeviceBam b;
        try { palace_host::load_bam_device(ctx, a.bam, 1, b, nullptr); }
        catch (const std::exception &e) { throw Failure(a.bam + ": " + e.what()); }
        std::string mean;
        if (palace_host::first_depth(ctx, b.n_segs, b.d_tid, b.d_pos, b.d_len, b.target_len, mean, nullptr, nullptr, &depth_sum, &depth_cov) < 0)
            throw Failure(std::string("the depth per contig: ") + palace_last_error());
        depth_name = b.target_name;
    } else {
        int64_t l = 0;
        for (const sv row : lines_of(table_text)) {
            l++;
            const size_t t1 = row.find('\t'), t2 = t1 == sv::npos ? sv::npos : row.find('\t', t1 + 1);
            uint64_t v[2] = {0, 0};
            bool ok = t2 != sv::npos && t1 > 0;
            for (int c = 0; ok && c < 2; c++) {
                const size_t from = c ? t2 + 1 : t1 + 1, to = c ? row.size() : t2;
                ok = to > from && to - from <= 18;
                for (size_t k = from; ok && k < to; k++) { ok = row[k] >= '0' && row[k] <= '9'; v[c] = v[c] * 10 + static_cast<uint64_t>(row[k] - '0'); }
            }
            if (!ok) line_fault(a.depth_table, l, "not name, sum and covered positions");
            depth_name.emplace_back(row.substr(0, t1));
            depth_sum.push_back(v[0]);
            depth_cov.push_back(v[1]);
        }
    }
    tr.lap("depth per contig");

    // names -> rows of the index, on the device: the index's names first, so that a name's id is its first row
    std::vector<sv> strings(fai_name);
    for (const sv w : words.text) strings.push_back(w.empty() ? w : w.substr(0, w.size() - 1));
    for (const std::string &n : depth_name) strings.push_back(n);
    const std::vector<int32_t> id = palace_host::ids_of(ctx, strings);
    for (size_t k = 0; k < n_fai; k++)
        if (static_cast<size_t>(id[k]) != k) line_fault(fai_path, static_cast<int64_t>(k) + 1, "sequence name '" + std::string(fai_name[k]) + "' appears a second time");
    std::vector<int32_t> token(words.text.size(), -1);
    for (size_t w = 0; w < words.text.size(); w++) {
        const int32_t base = id[n_fai + w];
        if (static_cast<size_t>(base) >= n_fai) {
            if (!*cdup::token_fault(words.text[w])) fault[words.file[w]].at(words.line[w], "'" + std::string(strings[n_fai + w]) + "' is no sequence of the index");
            continue;
        }
        token[w] = base << 1 | (words.text[w].back() == '-');
    }
    std::vector<cdup::NameInfo> info(n_fai);
    std::vector<uint8_t> info_ok(n_fai);
    for (size_t k = 0; k < n_fai; k++) info_ok[k] = cdup::name_info(fai_name[k], &info[k]);
    for (size_t w = 0; w < token.size(); w++)
        if (token[w] >= 0 && !info_ok[static_cast<size_t>(token[w] >> 1)]) fault[words.file[w]].at(words.line[w], "'" + std::string(words.text[w]) + "' begins with EDGE and has no length in its name");
    for (int f = 0; f < 3; f++)
        if (fault[f].line) line_fault(*file_name[f], fault[f].line, fault[f].reason);
    std::vector<cdup::Depth> depth(n_fai);
    for (size_t t = 0; t < depth_name.size(); t++) {
        const size_t base = static_cast<size_t>(id[n_fai + words.text.size() + t]);
        if (base < n_fai && t < depth_sum.size()) depth[base] = cdup::Depth{depth_sum[t], depth_cov[t]};
    }
    auto path_of = [&](const Span &s) { return Path(token.begin() + static_cast<std::ptrdiff_t>(s.first), token.begin() + static_cast<std::ptrdiff_t>(s.first + s.count)); };
    tr.lap("names resolved");

    // what the device decides, and the host's surgery around it (corrected_dup_rules.hpp: decide)
    std::vector<Path> original, finals;
    for (const Span &s : cycle_rows) original.push_back(path_of(s));
    for (const Span &s : final_rows) finals.push_back(path_of(s));
    std::vector<std::pair<Path, Path>> cut_pairs;
    for (const auto &row : cut_rows) cut_pairs.emplace_back(path_of(row.first), path_of(row.second));
    OnDevice device{ctx, fai_len};
    const std::vector<Path> first = cdup::decide(device, original, finals, cut_pairs, depth, fai_len);
    tr.lap("paths decided");

    // the quota rule, the length filter, the text
    auto text_of = [&](int32_t t) { return std::string(fai_name[static_cast<size_t>(t >> 1)]) + ((t & 1) ? '-' : '+'); };
    std::string out, warnings;
    for (const Path &p : first) {
        const Path q = cdup::quota(p, info, [&](int32_t t) {
            warnings += "Warning: Could not parse node: " + text_of(t) + ". Error: could not convert string to float: '" + info[static_cast<size_t>(t >> 1)].cov_text + "'\n";
        });
        if (cdup::written_length(q, info) <= a.min_len) continue;
        for (size_t k = 0; k < q.size(); k++) { if (k) out += '\t'; out += text_of(q[k]); }
        out += '\n';
    }
    std::error_code ec;
    std::filesystem::create_directories(a.out_dir, ec);
    const std::string out_path = (std::filesystem::path(a.out_dir) / a.out_name).string(), nodup_path = (std::filesystem::path(a.out_dir) / a.nodup_name).string();
    palace_host::PendingOutputs outputs;
    std::FILE *f = outputs.open(out_path);
    if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) throw Failure("cannot write " + out_path);
    outputs.open(nodup_path);
    if (!outputs.commit()) throw Failure("cannot write " + out_path);
    std::fputs(warnings.c_str(), stdout);
    tr.lap("output written");
}

}  // namespace

int main(int argc, char **argv)
{
    Args a;
    if (!parse_args(argc, argv, &a)) {
        std::fputs("usage: corrected_dup [--contig-depth table] out_dir prefix cycle_file final_all_file final.txt final.fasta edge_fasta cycle_nodup.txt bam before_cut min_len\n", stderr);
        return 2;
    }
    return palace_host::device_tool("corrected_dup", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, a, tr); });
}
