// readqc -- the first thing the driver does to a sample, which it gives to fastp (palace:358-363):
//     $FASTP -i fq1 -I fq2 -o out1 -O out2 -w N -j report.json -h report.html
// as  readqc -i fq1 -I fq2 -o out1 -O out2 -w N -j report.json -h report.html       (the argument list as the driver has it)
// Both FASTQ texts go up once; their lines are found (palace_sam_lines), their records validated (palace_fastq_records), every pair's
// overlap searched, trimmed and filtered (palace_readqc_plan) and the two output texts written in windows (palace_readqc_write) on
// the device (csrc/readqc.hip; the rules: DESIGN.md 8, csrc/fastq_rules.hpp).  The host reads the files and the command line and
// writes what comes back; no base is compared and no record is cut here.  fastp is not at hand: parity with it is UNPINNED.
//   A gzip input (told by its first two bytes; BGZF or not) is inflated on the device by palace_gzip_inflate, whose sink appends the
//   text to the buffer; where that declines the file, zlib inflates it on the host and decides it.
//   --full-report (readqc's own; needs -j): the JSON gets fastp's layout -- Q20/Q30, GC, read lengths, the per-cycle quality and
//   content curves of both reads before and after filtering, the insert sizes (DESIGN.md 8 "Reports").  Every count is the device's
//   (palace_readqc_plan_ex, palace_readqc_cycle_stats, palace_readqc_insert_sizes); the host divides and prints.  Without the option
//   the JSON is the ten integers it was.
//   Each output is written to <name>.tmp and renamed when both are complete; on any failure no file is left and stdout is empty.
// Needs a device: there is no host path.  The two texts, a pair of output windows and 96 B per pair (line starts, lengths, offsets) have
// to fit the device; else the `does not fit` message, and no way around it.  Exit 0; 1 for a text outside the grammar (`readqc:
// <path>: line N: <reason>` for the smallest faulty line, file 1 first) or any other failure; 2 for a usage error.
//   PALACE_READQC_WINDOW: bytes of output text per window (default 256 MiB); a window is copied back and written while the next one
//   is computed.  PALACE_DEVICE, PALACE_TRACE, PALACE_NO_FORK as in the other tools.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "trace.hpp"

namespace {

using palace_host::DeviceScope;
using palace_host::Failure;

const char *fault_text(int code)
{
    switch (code) {
    case PALACE_FASTQ_ELINES: return "the text ends inside a record (fewer than 4 lines)";
    case PALACE_FASTQ_EAT: return "a record's first line does not begin with '@'";
    case PALACE_FASTQ_EPLUS: return "a record's third line does not begin with '+'";
    case PALACE_FASTQ_ELONG: return "a read of more than 4096 bases";
    case PALACE_FASTQ_EBASE: return "a base other than A, C, G, T, N";
    case PALACE_FASTQ_EQLEN: return "the quality line has not the sequence's length";
    case PALACE_FASTQ_EQUAL: return "a quality byte outside 33 .. 126";
    }
    return "unknown fault";
}

struct Options {
    std::string in1, in2, out1, out2, json, html, command;
    bool full_report = false;
    palace_readqc_params prm{15, 40, 5, 15, 0, 0, 0, 30, 5, 20, 50, 0};
};

int usage(const std::string &why)
{
    std::fprintf(stderr,
                 "usage: readqc -i <in1.fq[.gz]> -I <in2.fq[.gz]> -o <out1.fq> -O <out2.fq> [-w <threads>] [-j <report.json>] [-h <report.html>]\n"
                 "              [--full-report]                                   (readqc's own; with -j: the QC report in fastp's JSON layout)\n"
                 "              [-q <quality 15>] [-u <percent 40>] [-n <N limit 5>] [-l <length 15>] [-A] [-Q] [-L]      (fastp's long forms too)\n"
                 "  fastp's defaults for paired input: overlap-based adapter trimming, quality, N and length filters (DESIGN.md 8).  Nothing else\n"
                 "  of fastp is taken: no polyG/polyX, quality cutting, base correction, UMI, dedup, merging, adapter sequences, single-end input\n"
                 "  or .gz output.\nreadqc: error: %s\n", why.c_str());
    return 2;
}

bool parse_int(const std::string &v, int lo, int hi, int32_t *out)
{
    if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    const long x = std::atol(v.c_str());
    if (x < lo || x > hi) return false;
    *out = static_cast<int32_t>(x);
    return true;
}

bool ends_with(const std::string &s, const char *tail)
{
    const size_t n = std::strlen(tail);
    return s.size() >= n && s.compare(s.size() - n, n, tail) == 0;
}

// ---- an input on the device --------------------------------------------------------------------------------------------------------
struct DeviceText { uint8_t *d = nullptr; int64_t n = 0; };

struct Grow {                                                                // the sink's side of palace_gzip_inflate: the text so far
    palace_ctx *ctx;
    DeviceScope *dev;
    uint8_t *d = nullptr;
    size_t cap = 0, n = 0;
    std::string error;
};
int take_text(void *user, const uint8_t *d_text, int64_t n, int)
{
    Grow &g = *static_cast<Grow *>(user);
    try {                                                                    // (nothing is thrown through the library's frames)
        const size_t need = g.n + static_cast<size_t>(n);
        if (need > g.cap) {
            const size_t cap = need > 2 * g.cap ? need : 2 * g.cap;
            uint8_t *d = g.dev->array<uint8_t>(cap, "a FASTQ text is read on the device and has no other path: it");
            palace_host::ck(palace_d2d(g.ctx, d, g.d, g.n), "palace_d2d");
            palace_host::ck(palace_sync(g.ctx), "palace_sync");
            if (g.d) g.dev->give_back(g.d);
            g.d = d; g.cap = cap;
        }
        palace_host::ck(palace_d2d(g.ctx, g.d + g.n, d_text, static_cast<size_t>(n)), "palace_d2d");
        palace_host::ck(palace_sync(g.ctx), "palace_sync");                  // (the library's text is valid until the sink returns)
        g.n = need;
        return 0;
    } catch (const std::exception &e) { g.error = e.what(); return 1; }
}

// every member of a gzip file by zlib; a damaged file is zlib's verdict
std::vector<uint8_t> inflate_on_host(const std::string &path, const uint8_t *file, size_t size)
{
    std::vector<uint8_t> text;
    z_stream z{};
    if (inflateInit2(&z, 15 + 16) != Z_OK) throw Failure("zlib: inflateInit2 failed");
    struct End { z_stream *z; ~End() { inflateEnd(z); } } end{&z};
    std::vector<uint8_t> buf(1u << 22);
    size_t at = 0;
    for (;;) {
        if (z.avail_in == 0 && at < size) {
            const size_t give = size - at < (1u << 30) ? size - at : (1u << 30);
            z.next_in = const_cast<Bytef *>(file + at);
            z.avail_in = static_cast<uInt>(give);
            at += give;
        }
        z.next_out = buf.data();
        z.avail_out = static_cast<uInt>(buf.size());
        const int rc = inflate(&z, Z_NO_FLUSH);
        text.insert(text.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
        if (rc == Z_STREAM_END) {                                            // a member's end: the file's, or the next member's header follows
            if (z.avail_in == 0 && at >= size) return text;
            if (inflateReset(&z) != Z_OK) throw Failure(path + ": zlib: inflateReset failed");
        } else if (rc == Z_BUF_ERROR) throw Failure(path + ": zlib: unexpected end of file");            // (no input is left and the member is not done)
        else if (rc != Z_OK) throw Failure(path + ": zlib: " + (z.msg ? z.msg : "the gzip data is damaged"));
    }
}

DeviceText load_text(palace_ctx *ctx, DeviceScope &dev, const std::string &path, palace_host::Trace &tr)
{
    palace_host::MappedText file;
    palace_host::open_text(file, path);
    DeviceText t;
    if (file.size >= 2 && file.bytes()[0] == 0x1f && file.bytes()[1] == 0x8b) {
        Grow g{ctx, &dev};
        palace_gzip_stats st{};
        const palace_gzip_params prm{0, 0, 0, 0};
        const int rc = palace_gzip_inflate(ctx, file.bytes(), static_cast<int64_t>(file.size), &prm, take_text, &g, &st);
        if (!g.error.empty()) throw Failure(g.error);
        if (rc != PALACE_OK) throw Failure(std::string("palace_gzip_inflate failed: ") + palace_last_error());
        if (st.fallback == 0) { t.d = g.d ? g.d : dev.array<uint8_t>(0, "an empty text"); t.n = static_cast<int64_t>(g.n); tr.lap("input inflated (device)"); return t; }
        if (g.d) dev.give_back(g.d);                                         // (what the sink took is void: zlib decides the file)
        const std::vector<uint8_t> text = inflate_on_host(path, file.bytes(), file.size);
        t.d = dev.upload(text.data(), text.size(), "a FASTQ text is read on the device and has no other path: it");
        t.n = static_cast<int64_t>(text.size());
        tr.lap("input inflated (zlib), uploaded");
        return t;
    }
    t.d = dev.upload(file.bytes(), file.size, "a FASTQ text is read on the device and has no other path: it");
    t.n = static_cast<int64_t>(file.size);
    tr.lap("input uploaded");
    return t;
}

struct Lines { int64_t *d_start = nullptr; int64_t n_lines = 0, records = 0, bad_line = 0; int32_t code = 0, longest = 0; };

// longest: the longest read, for the report's cycle tables (asked for only then: the lengths come back, 4 bytes a read)
Lines lines_and_records(palace_ctx *ctx, DeviceScope &dev, const DeviceText &t, bool want_longest)
{
    Lines l;
    const palace_host::TextLines tl = palace_host::text_lines(ctx, dev, t.d, t.n, "the line starts");       // (the verdict in tl.res is a SAM's: it means nothing here)
    l.n_lines = tl.n_lines;
    l.d_start = tl.d_start;
    int32_t *d_seq_len = dev.array<int32_t>(static_cast<size_t>(l.n_lines / 4), "the reads' lengths");
    int64_t v[3];
    HIP_OK(palace_fastq_records(ctx, t.d, l.d_start, l.n_lines, d_seq_len, v));
    if (want_longest && v[2] == 0 && v[0] > 0) {
        std::vector<int32_t> seq_len(static_cast<size_t>(v[0]));
        HIP_OK(palace_d2h(ctx, seq_len.data(), d_seq_len, seq_len.size() * sizeof(int32_t)));
        for (const int32_t n : seq_len) l.longest = n > l.longest ? n : l.longest;
    }
    dev.give_back(d_seq_len);
    l.records = v[0]; l.bad_line = v[1]; l.code = static_cast<int32_t>(v[2]);
    return l;
}

// ---- the full report -----------------------------------------------------------------------------------------------------------------
// What the device counted: the plan's sums, the four sections of the two cycle_stats calls and the histogram.  Nothing is counted here.
struct Section {                                                             // one section of palace_readqc_cycle_stats, as it lies in d_out
    const uint64_t *w;
    int32_t max_cycles;
    uint64_t cnt(int32_t c, int slot) const { return w[static_cast<size_t>(c) * PALACE_READQC_SLOTS + slot]; }
    uint64_t qsum(int32_t c, int slot) const { return w[static_cast<size_t>(max_cycles + c) * PALACE_READQC_SLOTS + slot]; }
    uint64_t q20() const { return w[2 * static_cast<size_t>(max_cycles) * PALACE_READQC_SLOTS]; }
    uint64_t q30() const { return w[2 * static_cast<size_t>(max_cycles) * PALACE_READQC_SLOTS + 1]; }
    uint64_t at(int32_t c) const { uint64_t s = 0; for (int k = 0; k < PALACE_READQC_SLOTS; k++) s += cnt(c, k); return s; }
    uint64_t bases() const { uint64_t s = 0; for (int32_t c = 0; c < max_cycles; c++) s += at(c); return s; }
    uint64_t gc() const { uint64_t s = 0; for (int32_t c = 0; c < max_cycles; c++) s += cnt(c, 1) + cnt(c, 2); return s; }
    int32_t cycles() const { int32_t n = max_cycles; while (n > 0 && at(n - 1) == 0) n--; return n; }       // the longest read of the section
};
struct FullCounts {
    std::vector<uint64_t> stats[2], hist;                                    // per text: before, after; the 513 insert-size slots
    int32_t max_cycles[2] = {0, 0};
    Section section(int text, int after) const
    {
        return Section{stats[text].data() + static_cast<size_t>(after) * PALACE_READQC_SECTION_WORDS(max_cycles[text]), max_cycles[text]};
    }
};

double ratio(uint64_t num, uint64_t den) { return den ? static_cast<double>(num) / static_cast<double>(den) : 0.0; }
std::string num(uint64_t v) { return std::to_string(v); }
std::string num(double v)                                                    // 17 digits: a parser reads back the double that was computed
{
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}
std::string quoted(const std::string &s)
{
    std::string q = "\"";
    for (const char ch : s) {
        const unsigned char c = static_cast<unsigned char>(ch);
        if (c == '"' || c == '\\') { q += '\\'; q += ch; }
        else if (c < 0x20) { char b[8]; std::snprintf(b, sizeof b, "\\u%04x", c); q += b; }
        else q += ch;
    }
    return q + "\"";
}
template <class F> std::string curve(const char *name, int32_t cycles, F value)
{
    std::string s = std::string("\t\t\t\"") + name + "\":[";
    for (int32_t c = 0; c < cycles; c++) s += (c ? "," : "") + num(value(c));
    return s + "]";
}

std::string read_block(const char *name, const Section &x, uint64_t reads)
{
    static const struct { const char *name; int slot; } kBases[] = {{"A", 0}, {"T", 3}, {"C", 1}, {"G", 2}, {"N", 4}};
    const int32_t cycles = x.cycles();
    std::string s = std::string("\t\"") + name + "\": {\n\t\t\"total_reads\":" + num(reads) + ",\n\t\t\"total_bases\":" + num(x.bases()) + ",\n\t\t\"q20_bases\":" +
                    num(x.q20()) + ",\n\t\t\"q30_bases\":" + num(x.q30()) + ",\n\t\t\"total_cycles\":" + num(static_cast<uint64_t>(cycles)) + ",\n\t\t\"quality_curves\": {\n";
    for (int b = 0; b < 4; b++) s += curve(kBases[b].name, cycles, [&](int32_t c) { return ratio(x.qsum(c, kBases[b].slot), x.cnt(c, kBases[b].slot)); }) + ",\n";
    s += curve("mean", cycles, [&](int32_t c) { uint64_t q = 0; for (int k = 0; k < PALACE_READQC_SLOTS; k++) q += x.qsum(c, k); return ratio(q, x.at(c)); }) + "\n\t\t},\n";
    s += "\t\t\"content_curves\": {\n";
    for (int b = 0; b < 5; b++) s += curve(kBases[b].name, cycles, [&](int32_t c) { return ratio(x.cnt(c, kBases[b].slot), x.at(c)); }) + ",\n";
    s += curve("GC", cycles, [&](int32_t c) { return ratio(x.cnt(c, 1) + x.cnt(c, 2), x.at(c)); }) + "\n\t\t}\n\t}";
    return s;
}

std::string summary_block(const char *name, const Section &one, const Section &two, uint64_t reads_each)
{
    const uint64_t b1 = one.bases(), b2 = two.bases(), bases = b1 + b2, q20 = one.q20() + two.q20(), q30 = one.q30() + two.q30();
    return std::string("\t\t\"") + name + "\": {\n\t\t\t\"total_reads\":" + num(2 * reads_each) + ",\n\t\t\t\"total_bases\":" + num(bases) + ",\n\t\t\t\"q20_bases\":" + num(q20) +
           ",\n\t\t\t\"q30_bases\":" + num(q30) + ",\n\t\t\t\"q20_rate\":" + num(ratio(q20, bases)) + ",\n\t\t\t\"q30_rate\":" + num(ratio(q30, bases)) +
           ",\n\t\t\t\"read1_mean_length\":" + num(reads_each ? b1 / reads_each : 0) + ",\n\t\t\t\"read2_mean_length\":" + num(reads_each ? b2 / reads_each : 0) +
           ",\n\t\t\t\"gc_content\":" + num(ratio(one.gc() + two.gc(), bases)) + "\n\t\t}";
}

std::string full_report(const Options &o, const int64_t *n, const FullCounts &f)
{
    const auto plan = [&](int k) { return num(static_cast<uint64_t>(n[k])); };
    const uint64_t pairs = static_cast<uint64_t>(n[PALACE_READQC_READS_BEFORE]) / 2, kept = static_cast<uint64_t>(n[PALACE_READQC_READS_AFTER]) / 2;
    const Section before[2] = {f.section(0, 0), f.section(1, 0)}, after[2] = {f.section(0, 1), f.section(1, 1)};
    std::string s = "{\n\t\"summary\": {\n\t\t\"readqc_version\": " + quoted(palace_version()) + ",\n\t\t\"sequencing\": \"paired end (" +
                    std::to_string(before[0].cycles()) + " cycles + " + std::to_string(before[1].cycles()) + " cycles)\",\n";
    s += summary_block("before_filtering", before[0], before[1], pairs) + ",\n" + summary_block("after_filtering", after[0], after[1], kept) + "\n\t},\n";
    s += "\t\"filtering_result\": {\n\t\t\"passed_filter_reads\": " + plan(PALACE_READQC_READS_AFTER) + ",\n\t\t\"low_quality_reads\": " + plan(PALACE_READQC_LOW_QUALITY) +
         ",\n\t\t\"too_many_N_reads\": " + plan(PALACE_READQC_TOO_MANY_N) + ",\n\t\t\"too_short_reads\": " + plan(PALACE_READQC_TOO_SHORT) +
         ",\n\t\t\"too_long_reads\": 0\n\t},\n";
    s += "\t\"adapter_cutting\": {\n\t\t\"adapter_trimmed_reads\": " + plan(PALACE_READQC_TRIMMED_READS) + ",\n\t\t\"adapter_trimmed_bases\": " +
         plan(PALACE_READQC_TRIMMED_BASES) + "\n\t},\n";
    int peak = 0;                                                            // the smallest index of the largest count among 0 .. 511
    for (int k = 1; k < PALACE_READQC_ISIZE_MAX; k++)
        if (f.hist[static_cast<size_t>(k)] > f.hist[static_cast<size_t>(peak)]) peak = k;
    s += "\t\"insert_size\": {\n\t\t\"peak\": " + std::to_string(peak) + ",\n\t\t\"unknown\": " + num(f.hist[PALACE_READQC_ISIZE_MAX]) + ",\n\t\t\"histogram\":[";
    for (int k = 0; k < PALACE_READQC_ISIZE_MAX; k++) s += (k ? "," : "") + num(f.hist[static_cast<size_t>(k)]);
    s += "]\n\t},\n";
    s += read_block("read1_before_filtering", before[0], pairs) + ",\n" + read_block("read2_before_filtering", before[1], pairs) + ",\n" +
         read_block("read1_after_filtering", after[0], kept) + ",\n" + read_block("read2_after_filtering", after[1], kept) + ",\n";
    return s + "\t\"command\": " + quoted(o.command) + "\n}\n";
}

void write_report(const Options &o, const int64_t *n, const FullCounts *full)
{
    if (full) {
        const std::string text = full_report(o, n, *full);
        std::FILE *f = std::fopen(o.json.c_str(), "wb");
        if (!f) throw Failure("cannot write " + o.json);
        const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
        if ((std::fclose(f) != 0) | !ok) throw Failure("cannot write " + o.json);
    } else if (!o.json.empty()) {
        std::FILE *f = std::fopen(o.json.c_str(), "wb");
        if (!f) throw Failure("cannot write " + o.json);
        std::fprintf(f,
                     "{\n\t\"summary\": {\n\t\t\"before_filtering\": {\n\t\t\t\"total_reads\":%lld,\n\t\t\t\"total_bases\":%lld\n\t\t},\n"
                     "\t\t\"after_filtering\": {\n\t\t\t\"total_reads\":%lld,\n\t\t\t\"total_bases\":%lld\n\t\t}\n\t},\n"
                     "\t\"filtering_result\": {\n\t\t\"passed_filter_reads\": %lld,\n\t\t\"low_quality_reads\": %lld,\n\t\t\"too_many_N_reads\": %lld,\n"
                     "\t\t\"too_short_reads\": %lld\n\t},\n"
                     "\t\"adapter_cutting\": {\n\t\t\"adapter_trimmed_reads\": %lld,\n\t\t\"adapter_trimmed_bases\": %lld\n\t}\n}\n",
                     static_cast<long long>(n[PALACE_READQC_READS_BEFORE]), static_cast<long long>(n[PALACE_READQC_BASES_BEFORE]),
                     static_cast<long long>(n[PALACE_READQC_READS_AFTER]), static_cast<long long>(n[PALACE_READQC_BASES_AFTER]),
                     static_cast<long long>(n[PALACE_READQC_READS_AFTER]), static_cast<long long>(n[PALACE_READQC_LOW_QUALITY]),
                     static_cast<long long>(n[PALACE_READQC_TOO_MANY_N]), static_cast<long long>(n[PALACE_READQC_TOO_SHORT]),
                     static_cast<long long>(n[PALACE_READQC_TRIMMED_READS]), static_cast<long long>(n[PALACE_READQC_TRIMMED_BASES]));
        if (std::fclose(f) != 0) throw Failure("cannot write " + o.json);
    }
    if (!o.html.empty()) {
        std::FILE *f = std::fopen(o.html.c_str(), "wb");
        if (!f) throw Failure("cannot write " + o.html);
        std::fprintf(f, "<html><body><p>readqc report: see %s</p></body></html>\n", o.json.empty() ? "(no JSON report was asked for)" : o.json.c_str());
        if (std::fclose(f) != 0) throw Failure("cannot write " + o.html);
    }
}

void run(palace_ctx *ctx, const Options &o, palace_host::Trace &tr)
{
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const std::string *in[2] = {&o.in1, &o.in2}, *outp[2] = {&o.out1, &o.out2};
    DeviceText text[2];
    Lines lines[2];
    for (int k = 0; k < 2; k++) text[k] = load_text(ctx, dev, *in[k], tr);
    for (int k = 0; k < 2; k++) lines[k] = lines_and_records(ctx, dev, text[k], o.full_report);
    tr.lap("lines cut, records validated");
    for (int k = 0; k < 2; k++)
        if (lines[k].code) throw Failure(*in[k] + ": line " + std::to_string(lines[k].bad_line) + ": " + fault_text(lines[k].code));
    if (lines[0].records != lines[1].records)
        throw Failure(o.in2 + ": " + std::to_string(lines[1].records) + " records, but " + o.in1 + " has " + std::to_string(lines[0].records));

    const int64_t n_pairs = lines[0].records;
    const size_t np = static_cast<size_t>(n_pairs);
    int32_t *d_len[2] = {dev.array<int32_t>(np, "the kept lengths"), dev.array<int32_t>(np, "the kept lengths")};
    int64_t *d_off[2] = {dev.array<int64_t>(np + 1, "the records' places"), dev.array<int64_t>(np + 1, "the records' places")};
    int32_t *d_cand = o.full_report ? dev.array<int32_t>(np, "the pairs' candidates") : nullptr;
    int64_t n[PALACE_READQC_N_OUT];
    HIP_OK(palace_readqc_plan_ex(ctx, text[0].d, lines[0].d_start, text[1].d, lines[1].d_start, n_pairs, &o.prm, d_len[0], d_len[1], d_off[0], d_off[1], d_cand, n));
    tr.lap("pairs planned");

    FullCounts full;
    if (o.full_report) {                                                     // the report's counts: two cycle_stats calls and the histogram, then one wait
        uint64_t *d_stats[2], *d_hist = dev.array<uint64_t>(PALACE_READQC_ISIZE_MAX + 1, "the insert sizes");
        for (int k = 0; k < 2; k++) {
            full.max_cycles[k] = lines[k].longest;
            full.stats[k].resize(2 * static_cast<size_t>(PALACE_READQC_SECTION_WORDS(full.max_cycles[k])));
            d_stats[k] = dev.array<uint64_t>(full.stats[k].size(), "the cycle tables");
            HIP_OK(palace_readqc_cycle_stats(ctx, text[k].d, lines[k].d_start, n_pairs, d_len[k], full.max_cycles[k], d_stats[k]));
        }
        HIP_OK(palace_readqc_insert_sizes(ctx, lines[0].d_start, lines[1].d_start, d_cand, n_pairs, &o.prm, d_hist));
        full.hist.resize(PALACE_READQC_ISIZE_MAX + 1);
        for (int k = 0; k < 2; k++) HIP_OK(palace_d2h(ctx, full.stats[k].data(), d_stats[k], full.stats[k].size() * sizeof(uint64_t)));
        HIP_OK(palace_d2h(ctx, full.hist.data(), d_hist, full.hist.size() * sizeof(uint64_t)));
        for (int k = 0; k < 2; k++) dev.give_back(d_stats[k]);
        dev.give_back(d_hist);
        dev.give_back(d_cand);
        tr.lap("report counted");
    }

    // windows of the output texts: window w is computed and copied back while window w - 1 goes to its file
    const int64_t total[2] = {n[PALACE_READQC_BYTES_1], n[PALACE_READQC_BYTES_2]};
    palace_host::WindowWriter windows(ctx, dev, "PALACE_READQC_WINDOW", total[0] > total[1] ? total[0] : total[1]);
    palace_host::PendingOutputs outputs;
    for (int k = 0; k < 2; k++) {
        std::FILE *f = outputs.open(*outp[k]);
        windows.write(total[k], f, *outp[k] + ".tmp", [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_readqc_write(ctx, text[k].d, lines[k].d_start, d_len[k], d_off[k], n_pairs, lo, hi, d_win));
        });
    }
    if (const std::string *bad = outputs.close()) throw Failure("cannot write " + *bad);
    tr.lap("outputs written");
    write_report(o, n, o.full_report ? &full : nullptr);
    if (const std::string *bad = outputs.rename()) throw Failure("cannot rename " + *bad);
    if (tr.on)
        std::fprintf(stderr, "[readqc] pairs %lld, kept %lld; text %lld + %lld B in, %lld + %lld B out; build %s\n", static_cast<long long>(n_pairs),
                     static_cast<long long>(n[PALACE_READQC_READS_AFTER] / 2), static_cast<long long>(text[0].n), static_cast<long long>(text[1].n),
                     static_cast<long long>(total[0]), static_cast<long long>(total[1]), palace_version());
}

}  // namespace

int main(int argc, char **argv)
{
    Options o;
    struct Valued { const char *shrt, *lng; std::string *text; int32_t *num; int lo, hi; };
    int32_t threads = 0;
    const Valued valued[] = {{"-i", "--in1", &o.in1, nullptr, 0, 0}, {"-I", "--in2", &o.in2, nullptr, 0, 0}, {"-o", "--out1", &o.out1, nullptr, 0, 0},
                             {"-O", "--out2", &o.out2, nullptr, 0, 0}, {"-j", "--json", &o.json, nullptr, 0, 0}, {"-h", "--html", &o.html, nullptr, 0, 0},
                             {"-w", "--thread", nullptr, &threads, 0, 1 << 20}, {"-q", "--qualified_quality_phred", nullptr, &o.prm.qualified_quality, 0, 93},
                             {"-u", "--unqualified_percent_limit", nullptr, &o.prm.unqualified_percent, 0, 100},
                             {"-n", "--n_base_limit", nullptr, &o.prm.n_limit, 0, 1 << 20}, {"-l", "--length_required", nullptr, &o.prm.min_length, 0, 1 << 20}};
    struct Flag { const char *shrt, *lng; int32_t *on; };
    const Flag flags[] = {{"-A", "--disable_adapter_trimming", &o.prm.no_trim}, {"-Q", "--disable_quality_filtering", &o.prm.no_quality_filter},
                          {"-L", "--disable_length_filtering", &o.prm.no_length_filter}};
    for (int i = 1; i < argc; i++) o.command += std::string(i > 1 ? " " : "") + argv[i];
    o.command = std::string("readqc") + (argc > 1 ? " " : "") + o.command;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        bool taken = false;
        if (a == "--full-report") { o.full_report = taken = true; }
        for (const Flag &f : flags)
            if (a == f.shrt || a == f.lng) { *f.on = 1; taken = true; }
        for (const Valued &v : valued) {
            if (taken) break;
            std::string value;
            const std::string lng_eq = std::string(v.lng) + "=";
            if (a == v.shrt || a == v.lng) {
                if (i + 1 >= argc) return usage("option " + a + " needs a value");
                value = argv[++i];
            } else if (a.compare(0, lng_eq.size(), lng_eq) == 0) value = a.substr(lng_eq.size());
            else continue;
            taken = true;
            if (v.text) {
                if (value.empty()) return usage("option " + a + " needs a value");
                *v.text = value;
            } else if (!parse_int(value, v.lo, v.hi, v.num))
                return usage("option " + a + ": '" + value + "' is not a number in " + std::to_string(v.lo) + " .. " + std::to_string(v.hi));
        }
        if (!taken) return usage("option " + a + " is not taken");
    }
    if (o.in1.empty() || o.in2.empty() || o.out1.empty() || o.out2.empty()) return usage("-i, -I, -o and -O are required (paired input only)");
    if (ends_with(o.out1, ".gz") || ends_with(o.out2, ".gz")) return usage(".gz output is not written");
    if (o.full_report && o.json.empty()) return usage("--full-report needs -j: the report is the JSON file");

    return palace_host::device_tool("readqc", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, o, tr); });
}
