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
#include "fast_exit.hpp"
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "textio.hpp"
#include "trace.hpp"

namespace {

using palace_host::DeviceScope;
using palace_host::Failure;
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

[[noreturn]] void fault(const std::string &file, int64_t line, const std::string &reason)
{
    throw Failure(file + ": line " + std::to_string(line) + ": " + reason);
}

void open_text(palace_host::MappedText &t, const std::string &path)
{
    try { t.open(path); }
    catch (const std::exception &) { throw Failure("cannot open " + path); }
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
    std::vector<int32_t> rec(strings.size(), -1);
    if (strings.empty()) return rec;
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const uint8_t *d_text = dev.upload(reinterpret_cast<const uint8_t *>(text.data()), text.size(), "the names of the hit and score files");
    const int64_t *d_off = dev.upload(off.data(), off.size(), "the names' offsets");
    int32_t *d_code = dev.array<int32_t>(strings.size(), "the names' records");
    HIP_OK(palace_path_resolve(ctx, names, d_text, d_off, static_cast<int64_t>(strings.size()), d_code));
    HIP_OK(palace_d2h(ctx, rec.data(), d_code, rec.size() * sizeof(int32_t)));
    for (int32_t &c : rec) c = (c < 0 || (c & PALACE_PATH_SECOND_TRY)) ? -1 : c >> 2;
    return rec;
}

void run(palace_ctx *ctx, const Args &a, palace_host::Trace &tr)
{
    palace_host::MappedText ftext, ptext, btext, htext, stext;
    open_text(ftext, a.fasta);
    open_text(ptext, a.paths);
    open_text(btext, a.blast);
    open_text(htext, a.hits);
    open_text(stext, a.scores);
    tr.lap("files read");

    // the assembly: text, index, names; two records of one name are a fault (the reference's to_dict raises)
    DeviceScope as(ctx, palace_host::no_room_does_not_fit);
    palace_host::FastaNamesHandle names(ctx);
    const int64_t fn = static_cast<int64_t>(ftext.size);
    const uint8_t *d_text = as.upload(ftext.bytes(), ftext.size, "the FASTA is read on the device and has no other path: it");
    const palace_host::FastaIndex ix = palace_host::index_fasta(ctx, as, d_text, fn, "the FASTA's index");
    if (ix.st.error) fault(a.fasta, ix.st.bad_line, palace_host::fasta_fault_text(ix.st.error));
    palace_fasta_rec *const d_recs = ix.d_recs;
    const int64_t n_rec = ix.st.n_records;
    {
        const std::vector<uint8_t> dup = palace_host::hash_names(ctx, as, d_text, d_recs, n_rec, names);
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

    // the BLAST table where it lies: lines, groups, one byte per record
    std::vector<uint8_t> bits(static_cast<size_t>(n_rec), 0);
    {
        DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
        const int64_t bn = static_cast<int64_t>(btext.size);
        const uint8_t *d_blast = dev.upload(btext.bytes(), btext.size, "the BLAST table is read on the device and has no other path: it");
        const size_t sb = palace_sam_scratch_bytes(bn);
        void *d_scratch = dev.alloc(sb, "the lines' scratch");
        int64_t lines[5], out[5], cut[palace::kBlastCuts];
        HIP_OK(palace_sam_lines(ctx, d_blast, bn, d_scratch, sb, nullptr, 0, lines));
        const int64_t n_lines = lines[0];
        int64_t *d_start = dev.array<int64_t>(static_cast<size_t>(n_lines) + 1, "the BLAST table's lines");
        HIP_OK(palace_sam_lines(ctx, d_blast, bn, d_scratch, sb, d_start, n_lines + 1, lines));
        uint8_t *d_seg = dev.array<uint8_t>(static_cast<size_t>(n_rec), "the records' bits");
        palace::blast_identity_cuts(a.ratio * 100.0, cut);
        HIP_OK(palace_blast_groups(ctx, d_blast, d_start, n_lines, names.h, n_rec, a.ratio, cut, d_seg, out));
        if (out[3]) fault(a.blast, out[3], palace::blast_line_error_text(static_cast<int32_t>(out[4])));
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
            if (cols.size() != 2 || cols[0].empty()) fault(a.scores, number, "not two columns");
            double v;
            if (!parse_number(cols[1], &v)) fault(a.scores, number, "a score that is not a decimal number");
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
    const uint8_t *d_tok = dev.upload(reinterpret_cast<const uint8_t *>(pt.text.data()), pt.text.size(), "the tokens");
    const int64_t *d_tok_off = dev.upload(pt.off.data(), pt.off.size(), "the tokens' offsets");
    int32_t *d_code = dev.array<int32_t>(static_cast<size_t>(n_tok), "the tokens' records");
    HIP_OK(palace_path_resolve(ctx, names.h, d_tok, d_tok_off, n_tok, d_code));
    {
        std::vector<int32_t> code(static_cast<size_t>(n_tok));
        if (n_tok) HIP_OK(palace_d2h(ctx, code.data(), d_code, code.size() * sizeof(int32_t)));
        for (int64_t p = 0; p < n_paths; p++)
            for (int64_t t = pt.tok_off[static_cast<size_t>(p)]; t < pt.tok_off[static_cast<size_t>(p) + 1]; t++)
                if (code[static_cast<size_t>(t)] < 0 || (code[static_cast<size_t>(t)] & PALACE_PATH_SECOND_TRY)) {
                    const sv tok = pt.token(t);
                    fault(a.paths, pt.line[static_cast<size_t>(p)], "name '" + std::string(tok.substr(0, tok.size() - 1)) + "' is no record of the FASTA");
                }
    }
    if (pt.bad_line) fault(a.paths, pt.bad_line, pt.bad_reason);
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
    std::string said, cycle, hdr;
    std::vector<int64_t> hdr_off{0}, path_out{0};
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
        int64_t bytes = 0;
        if (first[k] & PALACE_FILTERRES_WRITE) {
            hdr.append(joined);
            bytes = static_cast<int64_t>(joined.size()) + len[k] + 3;
        }
        hdr_off.push_back(static_cast<int64_t>(hdr.size()));
        path_out.push_back(path_out.back() + bytes);
    }
    const int64_t total = path_out.back();
    const uint8_t *d_hdr = dev.upload(reinterpret_cast<const uint8_t *>(hdr.data()), hdr.size(), "the headers");
    const int64_t *d_hdr_off = dev.upload(hdr_off.data(), hdr_off.size(), "the headers' offsets");
    const int64_t *d_path_out = dev.upload(path_out.data(), path_out.size(), "the paths' places");
    tr.lap("lengths and headers");

    // both outputs under other names until both are complete
    const std::string tmp = a.out + ".tmp", ctmp = a.cycle + ".tmp";
    std::FILE *out = std::fopen(tmp.c_str(), "wb");
    if (!out) throw Failure("cannot write " + tmp);
    palace_host::FileGuard closer{out, tmp.c_str()};
    if (total) {
        palace_host::WindowWriter windows(ctx, dev, "PALACE_FILTERRES_WINDOW", total);
        windows.write(total, out, tmp, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_final_fasta_write(ctx, d_text, d_recs, d_code, d_cum, d_path_off, n_paths, d_hdr, d_hdr_off, d_path_out, 'N', lo, hi, d_win));
        });
    }
    std::FILE *cf = std::fopen(ctmp.c_str(), "wb");
    if (!cf) throw Failure("cannot write " + ctmp);
    palace_host::FileGuard ccloser{cf, ctmp.c_str()};
    const bool wrote = std::fwrite(cycle.data(), 1, cycle.size(), cf) == cycle.size();
    closer.release();
    ccloser.release();
    const bool closed = (std::fclose(out) == 0) & (std::fclose(cf) == 0);
    if (!wrote || !closed || std::rename(tmp.c_str(), a.out.c_str()) != 0 || std::rename(ctmp.c_str(), a.cycle.c_str()) != 0) {
        std::remove(tmp.c_str());
        std::remove(ctmp.c_str());
        throw Failure("cannot write " + a.out + " and " + a.cycle);
    }
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
    palace_host::FastExit fast_exit = palace_host::fast_exit_begin();   // from here on this is the worker process (fast_exit.hpp)
    const int device = palace_host::pick_device();                       // PALACE_DEVICE (device_pick.hpp): before anything touches HIP
    palace_host::Trace tr("filter_result");
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(device, &ctx) != PALACE_OK) {
        std::fprintf(stderr, "filter_result: no GPU device to work on (%s); there is no CPU path\n", palace_last_error());
        return 1;
    }
    tr.lap("device up");
    try {
        run(ctx, a, tr);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "filter_result: %s\n", e.what());
        return 1;
    }
    fast_exit.done(0);          // both outputs are complete and renamed: the caller goes on, the teardown happens behind it
}
