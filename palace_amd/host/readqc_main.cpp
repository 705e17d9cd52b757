// readqc -- the first thing the driver does to a sample, which it gives to fastp (palace:358-363):
//     $FASTP -i fq1 -I fq2 -o out1 -O out2 -w N -j report.json -h report.html
// as  readqc -i fq1 -I fq2 -o out1 -O out2 -w N -j report.json -h report.html       (the argument list as the driver has it)
// Both FASTQ texts go up once; their lines are found (palace_sam_lines), their records validated (palace_fastq_records), every pair's
// overlap searched, trimmed and filtered (palace_readqc_plan) and the two output texts written in windows (palace_readqc_write) on
// the device (csrc/readqc.hip; the rules: DESIGN.md 8, csrc/fastq_rules.hpp).  The host reads the files and the command line and
// writes what comes back; no base is compared and no record is cut here.  fastp is not at hand: parity with it is UNPINNED.
//   A gzip input (told by its first two bytes; BGZF or not) is inflated on the device by palace_gzip_inflate, whose sink appends the
//   text to the buffer; where that declines the file, zlib inflates it on the host and decides it.
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
    std::string in1, in2, out1, out2, json, html;
    palace_readqc_params prm{15, 40, 5, 15, 0, 0, 0, 30, 5, 20, 50, 0};
};

int usage(const std::string &why)
{
    std::fprintf(stderr,
                 "usage: readqc -i <in1.fq[.gz]> -I <in2.fq[.gz]> -o <out1.fq> -O <out2.fq> [-w <threads>] [-j <report.json>] [-h <report.html>]\n"
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

struct Lines { int64_t *d_start = nullptr; int64_t n_lines = 0, records = 0, bad_line = 0; int32_t code = 0; };

Lines lines_and_records(palace_ctx *ctx, DeviceScope &dev, const DeviceText &t)
{
    Lines l;
    const palace_host::TextLines tl = palace_host::text_lines(ctx, dev, t.d, t.n, "the line starts");       // (the verdict in tl.res is a SAM's: it means nothing here)
    l.n_lines = tl.n_lines;
    l.d_start = tl.d_start;
    int32_t *d_seq_len = dev.array<int32_t>(static_cast<size_t>(l.n_lines / 4), "the reads' lengths");
    int64_t v[3];
    HIP_OK(palace_fastq_records(ctx, t.d, l.d_start, l.n_lines, d_seq_len, v));
    dev.give_back(d_seq_len);
    l.records = v[0]; l.bad_line = v[1]; l.code = static_cast<int32_t>(v[2]);
    return l;
}

void write_report(const Options &o, const int64_t *n)
{
    if (!o.json.empty()) {
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
    for (int k = 0; k < 2; k++) lines[k] = lines_and_records(ctx, dev, text[k]);
    tr.lap("lines cut, records validated");
    for (int k = 0; k < 2; k++)
        if (lines[k].code) throw Failure(*in[k] + ": line " + std::to_string(lines[k].bad_line) + ": " + fault_text(lines[k].code));
    if (lines[0].records != lines[1].records)
        throw Failure(o.in2 + ": " + std::to_string(lines[1].records) + " records, but " + o.in1 + " has " + std::to_string(lines[0].records));

    const int64_t n_pairs = lines[0].records;
    const size_t np = static_cast<size_t>(n_pairs);
    int32_t *d_len[2] = {dev.array<int32_t>(np, "the kept lengths"), dev.array<int32_t>(np, "the kept lengths")};
    int64_t *d_off[2] = {dev.array<int64_t>(np + 1, "the records' places"), dev.array<int64_t>(np + 1, "the records' places")};
    int64_t n[PALACE_READQC_N_OUT];
    HIP_OK(palace_readqc_plan(ctx, text[0].d, lines[0].d_start, text[1].d, lines[1].d_start, n_pairs, &o.prm, d_len[0], d_len[1], d_off[0], d_off[1], n));
    tr.lap("pairs planned");

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
    write_report(o, n);
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
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        bool taken = false;
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

    return palace_host::device_tool("readqc", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, o, tr); });
}
