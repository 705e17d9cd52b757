// filter_result <fasta> <all_result.txt> <filtered.fasta> <blast> <blast_ratio> <gene_hit> <node_score> <filtered_cycle.txt>: the
// reference's share/palace/scripts/filter_result.py (call site palace:604-612) with its argument list.  The FASTA's index and names,
// the BLAST table's groups, every path's class, the first-occurrence rule and the FASTA text are the device's (csrc/filter_result.hip,
// final_fasta.hip, path_fasta.hip; the rules: DESIGN.md 8).  The host reads the small files, splits the paths file into tokens, turns
// names into records through the name table on the device, and writes headers, stdout and the cycle file from the class bytes it
// copies back; it decides no class and produces no sequence byte.  There is no path around the device.
// PALACE_FILTERRES_WINDOW: bytes of output text per window (default 256 MiB), as PALACE_FINALFA_WINDOW of make_final_fa.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "../csrc/blast_line.hpp"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "textio.hpp"
#include "trace.hpp"

namespace {

using palace_host::DeviceScope;
using palace_host::Failure;
using palace_host::line_fault;
using palace_host::sv;

struct Args {
    std::string fasta, paths, out, blast, hits, scores, cycle;
    double ratio = 0;
};

// a decimal number as strtod and Python's float() both read it: digits, a point, an exponent; a leading '-' but no '+', no space
bool parse_number(sv s, double *out)
{
    if (s.empty() || !((s[0] >= '0' && s[0] <= '9') || s[0] == '.' || s[0] == '-')) return false;
    for (const char c : s)
        if (!((c >= '0' && c <= '9') || c == '.' || c == 'e' || c == 'E' || c == '+' || c == '-')) return false;
    const std::string z(s);
    char *end = nullptr;
    errno = 0;
    const double v = std::strtod(z.c_str(), &end);
    if (end != z.c_str() + z.size()) return false;
    *out = v;
    return true;
}

// The paths file: a line that begins with "self" or "iter" sets its tag for the rest of the file; any other line is stripped and,
// when something is left, cut at every TAB into tokens `name` `+|-`.  Reading stops at the first line outside the grammar.
struct Paths {
    std::vector<int64_t> line;                   // per path: its 1-based line
    std::vector<int64_t> tok_off{0};             // ... its tokens are tok_off[p] .. tok_off[p + 1]
    std::vector<uint8_t> tag;
    std::string text;                            // the tokens' bytes, one behind the other
    std::vector<int64_t> off{0};
    int64_t bad_line = 0;
    std::string bad_reason;
    sv token(int64_t t) const { return sv(text).substr(static_cast<size_t>(off[static_cast<size_t>(t)]), static_cast<size_t>(off[static_cast<size_t>(t) + 1] - off[static_cast<size_t>(t)])); }
};

std::string token_fault(sv tok)
{
    if (tok.size() < 2 || (tok.back() != '+' && tok.back() != '-')) return "token '" + std::string(tok) + "' is not a name followed by + or -";
    const sv name = tok.substr(0, tok.size() - 1);
    if (name.find_first_of("+- ") != sv::npos) return "token '" + std::string(tok) + "' is not a name followed by + or -";
    for (const char *word : {"ref", "self", "gene", "score", "cycle"})
        if (name.find(word) != sv::npos) return "name '" + std::string(name) + "' holds one of ref, self, gene, score, cycle";
    return "";
}

Paths split_paths(const char *p, size_t n)
{
    Paths out;
    uint8_t tag = 0;
    int64_t number = 0;
    palace_host::for_each_line(p, n, [&](sv raw) {
        number++;
        if (out.bad_line) return;
        const bool self = raw.substr(0, 4) == "self", iter = raw.substr(0, 4) == "iter";
        if (self || iter) { tag |= self ? PALACE_FILTERRES_TAG_SELF : PALACE_FILTERRES_TAG_CYCLE; return; }
        const sv s = palace_host::strip(raw);
        if (s.empty()) return;
        std::vector<sv> toks;
        palace_host::split_on(s, '\t', toks);
        for (const sv t : toks) {
            const std::string why = token_fault(t);
            if (!why.empty()) { out.bad_line = number; out.bad_reason = why; return; }
        }
        for (const sv t : toks) { out.text.append(t); out.off.push_back(static_cast<int64_t>(out.text.size())); }
        out.line.push_back(number);
        out.tag.push_back(tag);
        out.tok_off.push_back(static_cast<int64_t>(out.off.size()) - 1);
    });
    return out;
}

// names -> records through the FASTA's table on the device: -1 for a name that is no record.  A name that holds '+' or '-' never
// equals a token's name, and a code with PALACE_PATH_SECOND_TRY is not the name itself.
std::vector<int32_t> records_of(palace_ctx *ctx, const palace_fasta_names *names, const std::vector<sv> &strings)
{
    std::string text;
    std::vector<int64_t> off{0};
    for (const sv s : strings) {
        if (s.find_first_of("+-") == sv::npos) { text.append(s); text.push_back('+'); }
        off.push_back(static_cast<int64_t>(text.size()));
    }
    if (strings.empty()) return {};
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    std::vector<int32_t> rec = palace_host::resolve(ctx, dev, names, text, off, {"the names of the hit and score files", "the names' offsets", "the names' records", nullptr}, true).code;
    for (int32_t &c : rec) c = (c < 0 || (c & PALACE_PATH_SECOND_TRY)) ? -1 : c >> 2;
    return rec;
}

void run(palace_ctx *ctx, const Args &a, palace_host::Trace &tr)
{
    palace_host::Assembly as(ctx, a.fasta);
    palace_host::MappedText ptext, btext, htext, stext;
    palace_host::open_text(ptext, a.paths);
    palace_host::open_text(btext, a.blast);
    palace_host::open_text(htext, a.hits);
    palace_host::open_text(stext, a.scores);
    tr.lap("files read");

    // the assembly: text, index, names; two records of one name are a fault (the reference's to_dict raises)
    as.load(tr, [&](size_t, const palace_fasta_rec &r, const char *text) {
        line_fault(a.fasta, palace_host::line_of(text, r.name_off), "sequence name '" + std::string(text + r.name_off, static_cast<size_t>(r.name_len)) + "' appears a second time");
    });
    const uint8_t *const d_text = as.d_text;
    palace_fasta_rec *const d_recs = as.d_recs;
    const palace_host::FastaNamesHandle &names = as.names;
    const int64_t n_rec = as.n_records;

    // the BLAST table where it lies: lines, groups, one byte per record
    std::vector<uint8_t> bits(static_cast<size_t>(n_rec), 0);
    {
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const uint8_t *d_blast = dev.upload(btext.bytes(), btext.size, "the BLAST table is read on the device and has no other path: it");
        const palace_host::TextLines lines = palace_host::text_lines(ctx, dev, d_blast, static_cast<int64_t>(btext.size), "the BLAST table's lines");
        int64_t out[5], cut[palace::kBlastCuts];
        uint8_t *d_seg = dev.array<uint8_t>(static_cast<size_t>(n_rec), "the records' bits");
        palace::blast_identity_cuts(a.ratio * 100.0, cut);
        HIP_OK(palace_blast_groups(ctx, d_blast, lines.d_start, lines.n_lines, names.h, n_rec, a.ratio, cut, d_seg, out));
        if (out[3]) line_fault(a.blast, out[3], palace::blast_line_error_text(static_cast<int32_t>(out[4])));
        if (n_rec) HIP_OK(palace_d2h(ctx, bits.data(), d_seg, bits.size()));
        for (uint8_t &b : bits) b = b ? PALACE_FILTERRES_REC_BLAST : 0;
        tr.lap("BLAST groups");
    }

    // the hit list and the scores: a name's bits go to its record
    {
        std::vector<sv> name;
        std::vector<uint8_t> what;                                           // REC_GENE, or 0x80 | the score's bits
        std::vector<sv> cols;
        palace_host::for_each_line(htext.data, htext.size, [&](sv raw) {
            const sv s = palace_host::strip(raw);
            if (s.empty()) return;
            palace_host::split_on(s, '\t', cols);
            name.push_back(cols[0]);
            what.push_back(PALACE_FILTERRES_REC_GENE);
        });
        int64_t number = 0;
        palace_host::for_each_line(stext.data, stext.size, [&](sv raw) {
            number++;
            palace_host::split_on(palace_host::strip(raw), '\t', cols);
            if (cols.size() != 2 || cols[0].empty()) line_fault(a.scores, number, "not two columns");
            double v;
            if (!parse_number(cols[1], &v)) line_fault(a.scores, number, "a score that is not a decimal number");
            if (!(v >= 0.7)) return;                                         // (such a line does not reach the dict)
            name.push_back(cols[0]);
            what.push_back(static_cast<uint8_t>(0x80 | (v > 0.7 ? PALACE_FILTERRES_REC_S07 : 0) | (v >= 0.9 ? PALACE_FILTERRES_REC_S09 : 0)));
        });
        const std::vector<int32_t> rec = records_of(ctx, names.h, name);
        for (size_t k = 0; k < rec.size(); k++) {
            if (rec[k] < 0) continue;
            uint8_t &b = bits[static_cast<size_t>(rec[k])];
            if (what[k] & 0x80) b = static_cast<uint8_t>((b & ~(PALACE_FILTERRES_REC_S07 | PALACE_FILTERRES_REC_S09)) | (what[k] & 0x7f));   // the later line's score stays
            else b |= what[k];
        }
        tr.lap("hits and scores");
    }

    // the paths: tokens, records, the smallest faulty line
    const Paths pt = split_paths(ptext.data, ptext.size);
    const int64_t n_tok = static_cast<int64_t>(pt.off.size()) - 1, n_paths = static_cast<int64_t>(pt.line.size());
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    int32_t *d_code = nullptr;
    {
        const palace_host::Resolved res = palace_host::resolve(ctx, dev, names.h, pt.text, pt.off, palace_host::kTokensWhat, true);
        const std::vector<int32_t> &code = res.code;
        d_code = res.d_code;
        for (int64_t p = 0; p < n_paths; p++)
            for (int64_t t = pt.tok_off[static_cast<size_t>(p)]; t < pt.tok_off[static_cast<size_t>(p) + 1]; t++)
                if (code[static_cast<size_t>(t)] < 0 || (code[static_cast<size_t>(t)] & PALACE_PATH_SECOND_TRY)) {
                    const sv tok = pt.token(t);
                    line_fault(a.paths, pt.line[static_cast<size_t>(p)], "name '" + std::string(tok.substr(0, tok.size() - 1)) + "' is no record of the FASTA");
                }
    }
    if (pt.bad_line) line_fault(a.paths, pt.bad_line, pt.bad_reason);
    tr.lap("tokens resolved");

    // classes and the first of equal paths
    std::vector<uint8_t> cls(static_cast<size_t>(n_paths)), first(static_cast<size_t>(n_paths));
    std::vector<int64_t> all_len(static_cast<size_t>(n_paths));
    const int64_t *d_path_off = dev.upload(pt.tok_off.data(), pt.tok_off.size(), "the paths' tokens");
    {
        const uint8_t *d_tag = dev.upload(pt.tag.data(), pt.tag.size(), "the paths' tags");
        const uint8_t *d_bits = dev.upload(bits.data(), bits.size(), "the records' bits");
        uint8_t *d_cls = dev.array<uint8_t>(static_cast<size_t>(n_paths), "the paths' classes"), *d_first = dev.array<uint8_t>(static_cast<size_t>(n_paths), "the paths' classes");
        int64_t *d_all = dev.array<int64_t>(static_cast<size_t>(n_paths), "the paths' lengths");
        HIP_OK(palace_filter_result_plan(ctx, d_code, d_path_off, n_paths, d_tag, d_recs, d_bits, d_cls, d_all));
        HIP_OK(palace_paths_first_of_equal(ctx, d_code, d_path_off, n_paths, d_cls, 64, d_first));
        if (n_paths) {
            HIP_OK(palace_d2h(ctx, cls.data(), d_cls, cls.size()));
            HIP_OK(palace_d2h(ctx, first.data(), d_first, first.size()));
            HIP_OK(palace_d2h(ctx, all_len.data(), d_all, all_len.size() * sizeof(int64_t)));
        }
    }
    tr.lap("classes");

    // stdout, the cycle file and the headers, from the class bytes
    int64_t *d_cum = dev.array<int64_t>(static_cast<size_t>(n_tok + 1), "the tokens' places");
    int64_t *d_len = dev.array<int64_t>(static_cast<size_t>(n_paths), "the paths' lengths");
    HIP_OK(palace_final_fasta_lengths(ctx, d_recs, d_code, n_tok, d_path_off, n_paths, 0, d_cum, d_len));
    std::vector<int64_t> len(static_cast<size_t>(n_paths));
    if (n_paths) HIP_OK(palace_d2h(ctx, len.data(), d_len, len.size() * sizeof(int64_t)));
    std::string said, cycle;
    palace_host::PathsText plan;
    for (int64_t p = 0; p < n_paths; p++) {
        const size_t k = static_cast<size_t>(p);
        const sv joined = sv(pt.text).substr(static_cast<size_t>(pt.off[static_cast<size_t>(pt.tok_off[k])]),
                                             static_cast<size_t>(pt.off[static_cast<size_t>(pt.tok_off[k + 1])] - pt.off[static_cast<size_t>(pt.tok_off[k])]));
        const struct { int bit; const char *word; } words[] = {{PALACE_FILTERRES_SELFGENE, "selfgene"}, {PALACE_FILTERRES_CYCLEGENE, "cyclegene"},
                                                               {PALACE_FILTERRES_CYCLESCORE, "cyclescore"}, {PALACE_FILTERRES_GENESCORE, "genescore"}};
        for (const auto &w : words)
            if (cls[k] & w.bit) said.append(w.word).append(joined).push_back('\n');
        if (all_len[k] >= 10000)
            for (const int bit : {PALACE_FILTERRES_PLAIN, PALACE_FILTERRES_SELFGENE, PALACE_FILTERRES_CYCLEGENE, PALACE_FILTERRES_CYCLESCORE})
                if (first[k] & bit) cycle.append(bit >= PALACE_FILTERRES_CYCLEGENE ? "cycle" : "").append(joined).push_back('\n');
        if (first[k] & PALACE_FILTERRES_WRITE) plan.add(joined, len[k]);
        else plan.skip();
    }
    const palace_host::PathsText::OnDevice pd = plan.upload(dev);
    tr.lap("lengths and headers");

    // both outputs under other names until both are complete
    palace_host::PendingOutputs outputs;
    std::FILE *out = outputs.open(a.out);
    if (pd.total) {
        palace_host::WindowWriter windows(ctx, dev, "PALACE_FILTERRES_WINDOW", pd.total);
        windows.write(pd.total, out, a.out + ".tmp", [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_final_fasta_write(ctx, d_text, d_recs, d_code, d_cum, d_path_off, n_paths, pd.d_hdr, pd.d_hdr_off, pd.d_path_out, 'N', lo, hi, d_win));
        });
    }
    std::FILE *cf = outputs.open(a.cycle);
    const bool wrote = std::fwrite(cycle.data(), 1, cycle.size(), cf) == cycle.size();
    if (!wrote || !outputs.commit()) throw Failure("cannot write " + a.out + " and " + a.cycle);
    tr.lap("output written");
    std::fwrite(said.data(), 1, said.size(), stdout);
    std::fflush(stdout);
}

}  // namespace

int main(int argc, char **argv)
{
    Args a;
    if (argc != 9 || !parse_number(argv[5], &a.ratio)) {
        std::fputs("usage: filter_result fasta all_result.txt filtered.fasta blast blast_ratio gene_hit node_score filtered_cycle.txt\n", stderr);
        return 2;
    }
    a.fasta = argv[1]; a.paths = argv[2]; a.out = argv[3]; a.blast = argv[4]; a.hits = argv[6]; a.scores = argv[7]; a.cycle = argv[8];
    return palace_host::device_tool("filter_result", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, a, tr); });
}
