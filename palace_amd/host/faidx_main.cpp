// faidx [-n N] [-o OUT] [-r REGION_FILE] [-c] [-i] [--mark-strand rc|no|sign] <file.fa> [region ...]: the driver's `samtools faidx`
// calls (palace:403, 493, 702, 752: the index; palace:754, 770: one record by name), the FASTA indexed, the regions resolved and
// the output text gathered on the device (csrc/faidx.hip, path_fasta.hip, fastg_split.hip; the rules and the declared deviations:
// DESIGN.md 8).  samtools is absent where this was written: parity is UNPINNED, the rules are tests/faidx_cases.py's.
//   no region and no -r: <file.fa>.fai is written (as .tmp, renamed when complete); nothing on stdout.  A record whose name an
//   earlier record has is left out, with one warning line on stderr.
//   regions (the -r file's lines first, then the command line's): per region '>' region [mark] LF and its bases in lines of N
//   (default 60) to stdout or OUT (as OUT.tmp, renamed when complete).  No .fai is read or written.  A region that fails is
//   `[faidx] Failed to fetch sequence in <region>`: without -c for the first such region, exit 1 and no output byte; with -c for
//   each of them, in order, the others written, exit 0.
// The host reads the files, appends the strand mark to the headers and writes what comes back: it looks up no name, parses no
// coordinate and produces no sequence byte.  The FASTA, its index and two output windows have to fit the device: there is no path
// around it.  PALACE_FAIDX_WINDOW: bytes of output text per window (default 256 MiB).  Exit 2 for a usage error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "output_windows.hpp"
#include "trace.hpp"

namespace {

using palace_host::Failure;
using palace_host::DeviceScope;
using palace_host::Assembly;

struct Options {
    int64_t line_len = 60;
    std::string fasta, out, region_file, mark = "rc";
    bool have_out = false, have_region_file = false, keep_going = false, reverse = false;
    std::vector<std::string> regions;
};

void index_mode(palace_ctx *ctx, const Options &o, palace_host::Trace &tr)
{
    Assembly as(ctx, o.fasta);
    tr.lap("FASTA read");
    if (as.text.size >= 2 && as.text.bytes()[0] == 0x1f && as.text.bytes()[1] == 0x8b) throw Failure(o.fasta + ": compressed FASTA is not read");
    std::vector<uint8_t> skip;
    as.load(tr, [&](size_t k, const palace_fasta_rec &r, const char *text) {
        if (skip.empty()) skip.resize(static_cast<size_t>(as.n_records), 0);
        skip[k] = 1;
        std::fprintf(stderr, "faidx: warning: %s: sequence name '%.*s' appears again in record %zu: left out of %s.fai\n", o.fasta.c_str(),
                     static_cast<int>(r.name_len), text + r.name_off, k + 1, o.fasta.c_str());
    });
    const uint8_t *d_skip = skip.empty() ? nullptr : as.dev.upload(skip.data(), skip.size(), "the duplicate flags");
    palace_host::write_fai(ctx, as.d_text, as.d_recs, d_skip, as.n_records, o.fasta + ".fai", false);
    tr.lap("index rows written");
}

// the -r file's lines (a trailing CR is not the region's; a last line without LF is a line), then the command line's regions: one
// blob and its offsets
void read_regions(const Options &o, std::string &blob, std::vector<int64_t> &off)
{
    if (o.have_region_file) {
        palace_host::MappedText rt;
        palace_host::open_text(rt, o.region_file);
        for (size_t a = 0; a < rt.size;) {
            const void *lf = std::memchr(rt.data + a, '\n', rt.size - a);
            const size_t e = lf ? static_cast<size_t>(static_cast<const char *>(lf) - rt.data) : rt.size;
            blob.append(rt.data + a, e - a - ((e > a && rt.data[e - 1] == '\r') ? 1 : 0));
            off.push_back(static_cast<int64_t>(blob.size()));
            a = e + 1;
        }
    }
    for (const std::string &r : o.regions) { blob += r; off.push_back(static_cast<int64_t>(blob.size())); }
}

void fetch_mode(palace_ctx *ctx, const Options &o, palace_host::Trace &tr)
{
    Assembly as(ctx, o.fasta);
    tr.lap("FASTA read");
    if (as.text.size >= 2 && as.text.bytes()[0] == 0x1f && as.text.bytes()[1] == 0x8b) throw Failure(o.fasta + ": compressed FASTA is not read");
    std::string blob;
    std::vector<int64_t> off{0};
    read_regions(o, blob, off);
    const int64_t n_regions = static_cast<int64_t>(off.size()) - 1;
    tr.lap("regions read");
    as.load(tr, [](size_t, const palace_fasta_rec &, const char *) {});      // (of records with equal names the first is found)

    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const uint8_t *d_reg = dev.upload(reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), "the regions");
    const int64_t *d_reg_off = dev.upload(off.data(), off.size(), "the regions' offsets");
    palace_faidx_region *d_regions = dev.array<palace_faidx_region>(static_cast<size_t>(n_regions), "the regions' ranges");
    HIP_OK(palace_faidx_resolve(ctx, as.names.h, as.d_recs, d_reg, d_reg_off, n_regions, d_regions));

    // the headers: the regions themselves when no mark is appended
    const std::string mark = o.mark == "no" ? "" : o.mark == "sign" ? (o.reverse ? "(-)" : "(+)") : (o.reverse ? "/rc" : "");
    const uint8_t *d_hdr = d_reg;
    const int64_t *d_hdr_off = d_reg_off;
    if (!mark.empty()) {
        std::string hdr;
        std::vector<int64_t> hdr_off{0};
        hdr.reserve(blob.size() + mark.size() * static_cast<size_t>(n_regions));
        for (int64_t i = 0; i < n_regions; i++) {
            hdr.append(blob, static_cast<size_t>(off[static_cast<size_t>(i)]), static_cast<size_t>(off[static_cast<size_t>(i) + 1] - off[static_cast<size_t>(i)]));
            hdr += mark;
            hdr_off.push_back(static_cast<int64_t>(hdr.size()));
        }
        d_hdr = dev.upload(reinterpret_cast<const uint8_t *>(hdr.data()), hdr.size(), "the headers");
        d_hdr_off = dev.upload(hdr_off.data(), hdr_off.size(), "the headers' offsets");
    }
    int64_t *d_out_off = dev.array<int64_t>(static_cast<size_t>(n_regions) + 1, "the regions' places");
    int64_t total = 0, first_failed = -1;
    HIP_OK(palace_faidx_plan(ctx, d_regions, n_regions, d_hdr_off, o.line_len, o.keep_going ? 1 : 0, d_out_off, &total, &first_failed));
    tr.lap("regions resolved and planned");

    auto region = [&](int64_t i) { return blob.substr(static_cast<size_t>(off[static_cast<size_t>(i)]), static_cast<size_t>(off[static_cast<size_t>(i) + 1] - off[static_cast<size_t>(i)])); };
    if (first_failed >= 0 && !o.keep_going) {
        std::fprintf(stderr, "[faidx] Failed to fetch sequence in %s\n", region(first_failed).c_str());
        throw palace_host::SaidAlready();
    }
    {                                                                        // the lines of failed and of empty regions, in order
        std::vector<palace_faidx_region> regs(static_cast<size_t>(n_regions));
        if (n_regions) HIP_OK(palace_d2h(ctx, regs.data(), d_regions, regs.size() * sizeof(palace_faidx_region)));
        for (int64_t i = 0; i < n_regions; i++) {
            if (regs[static_cast<size_t>(i)].rec < 0) std::fprintf(stderr, "[faidx] Failed to fetch sequence in %s\n", region(i).c_str());
            else if (regs[static_cast<size_t>(i)].len == 0) std::fprintf(stderr, "[faidx] Zero length sequence: %s\n", region(i).c_str());
        }
    }

    palace_host::PendingOutputs outputs;
    std::FILE *out = o.have_out ? outputs.open(o.out) : stdout;
    const std::string out_name = o.have_out ? o.out + ".tmp" : "standard output";
    if (total) {                                                             // the output text, in windows (output_windows.hpp)
        palace_host::WindowWriter windows(ctx, dev, "PALACE_FAIDX_WINDOW", total);
        windows.write(total, out, out_name, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_faidx_write(ctx, as.d_text, as.d_recs, d_regions, n_regions, d_hdr, d_hdr_off, d_out_off, o.line_len, o.reverse ? 1 : 0, lo, hi, d_win));
        });
    }
    if (!o.have_out && std::fflush(stdout) != 0) throw Failure("cannot write standard output");
    if (const std::string *bad = outputs.close()) throw Failure("cannot write " + *bad);
    if (const std::string *bad = outputs.rename()) throw Failure("cannot write " + *bad);
    tr.lap("output written");
}

int usage(const std::string &why)
{
    std::fprintf(stderr, "usage: faidx [-n N] [-o OUT] [-r REGION_FILE] [-c] [-i] [--mark-strand rc|no|sign] <file.fa> [region ...]\nfaidx: error: %s\n",
                 why.c_str());
    return 2;
}

// N of -n: decimal digits, at least 1, at most 18 of them
bool line_length(const std::string &v, int64_t *out)
{
    if (v.empty() || v.size() > 18) return false;
    int64_t x = 0;
    for (const char c : v) {
        if (c < '0' || c > '9') return false;
        x = x * 10 + (c - '0');
    }
    *out = x;
    return x >= 1;
}

}  // namespace

int main(int argc, char **argv)
{
    Options o;
    std::vector<std::string> words;
    bool options_over = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (options_over || a.size() < 2 || a[0] != '-') { words.push_back(a); continue; }
        if (a == "--") { options_over = true; continue; }
        std::string name = a, value;
        bool have_value = false;
        if (a[1] == '-') {
            const size_t eq = a.find('=');
            if (eq != std::string::npos) { name = a.substr(0, eq); value = a.substr(eq + 1); have_value = true; }
        } else if (a.size() > 2) {                                           // -n60
            name = a.substr(0, 2); value = a.substr(2); have_value = true;
        }
        const bool takes = name == "-n" || name == "--length" || name == "-o" || name == "--output" || name == "-r" || name == "--region-file" ||
                           name == "--mark-strand";
        const bool flag = name == "-c" || name == "--continue" || name == "-i" || name == "--reverse-complement";
        if (name == "-f" || name == "--fastq" || name == "--fai-idx" || name == "--gzi-idx") return usage("option " + name + " is not supported");
        if (!takes && !flag) return usage("unrecognized option " + a);
        if (flag) {
            if (have_value) return usage("option " + name + " takes no value");
            if (name == "-c" || name == "--continue") o.keep_going = true; else o.reverse = true;
            continue;
        }
        if (!have_value) {
            if (i + 1 >= argc) return usage("option " + name + ": expected one argument");
            value = argv[++i];
        }
        if (name == "-n" || name == "--length") {
            if (!line_length(value, &o.line_len)) return usage("option " + name + ": the line length must be an integer >= 1");
        } else if (name == "-o" || name == "--output") { o.out = value; o.have_out = true; }
        else if (name == "-r" || name == "--region-file") { o.region_file = value; o.have_region_file = true; }
        else {
            if (value != "rc" && value != "no" && value != "sign") return usage("--mark-strand " + value + " is not supported (rc, no or sign)");
            o.mark = value;
        }
    }
    if (words.empty()) return usage("the FASTA file is required");
    o.fasta = words[0];
    o.regions.assign(words.begin() + 1, words.end());
    const bool fetch = o.have_region_file || !o.regions.empty();
    return palace_host::device_tool("faidx", [&](palace_ctx *ctx, palace_host::Trace &tr) {
        if (fetch) fetch_mode(ctx, o, tr); else index_mode(ctx, o, tr);
    });
}
