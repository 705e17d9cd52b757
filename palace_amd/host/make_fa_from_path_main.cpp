// make_fa_from_path <assembly.fasta> <paths> <out.fasta> <mode>: the reference's share/palace/scripts/make_fa_from_path.py (call
// sites palace:697-700, 747-750, 778-781) with its command line and its stdout, the FASTA indexed and the output text gathered
// on the device (csrc/path_fasta.hip; the rules: DESIGN.md 8).  The host reads the files, splits the paths file into tokens
// (path_tokens.hpp), writes the headers and the output file; no sequence byte is produced here.
//   make_fa_from_path --batch <list> <assembly.fasta>: one `<paths> <out.fasta> <mode>` per line of <list>; the FASTA is
//   uploaded, indexed and hashed once, every output is what a run of its own writes (the step-5 loop of palace:672-806).
// The FASTA has to fit the device whole: there is no path around the device.  PALACE_PATHFA_WINDOW: bytes of output text per
// window (default 256 MiB); a window is copied back and written to the file while the next one is computed.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "device_pick.hpp"
#include "device_scope.hpp"
#include "fast_exit.hpp"
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "output_windows.hpp"
#include "path_tokens.hpp"
#include "textio.hpp"
#include "trace.hpp"

namespace {

using palace_host::Failure;
using palace_host::DeviceScope;
using palace_host::fasta_fault_text;

// the assembly on the device: text, index, names
struct Assembly {
    palace_ctx *ctx;
    std::string path;
    palace_host::MappedText text;
    DeviceScope dev;
    palace_host::FastaNamesHandle names;
    const uint8_t *d_text = nullptr;
    palace_fasta_rec *d_recs = nullptr;
    int64_t n_records = 0;

    Assembly(palace_ctx *c, const std::string &fasta, palace_host::Trace &tr) : ctx(c), path(fasta), dev(c, palace_host::no_room_does_not_fit), names(c)
    {
        try { text.open(fasta); }
        catch (const std::exception &) { throw Failure("cannot open " + fasta); }
        tr.lap("FASTA read");
        const int64_t n = static_cast<int64_t>(text.size);
        d_text = dev.upload(text.bytes(), text.size, "the FASTA is read on the device and has no other path: it");
        tr.lap("FASTA uploaded");
        const palace_host::FastaIndex ix = palace_host::index_fasta(ctx, dev, d_text, n, "the FASTA's index");
        if (ix.st.error) throw Failure(fasta + ": line " + std::to_string(ix.st.bad_line) + ": " + fasta_fault_text(ix.st.error));
        d_recs = ix.d_recs;
        n_records = ix.st.n_records;
        tr.lap("FASTA indexed");
        const std::vector<uint8_t> h_dup = palace_host::hash_names(ctx, dev, d_text, d_recs, n_records, names);
        size_t k = 0;
        for (; k < h_dup.size() && !h_dup[k]; k++) {}
        if (k < h_dup.size()) {                                             // (rare: the records come to the host only to name them)
            std::vector<palace_fasta_rec> recs(h_dup.size());
            HIP_OK(palace_d2h(ctx, recs.data(), d_recs, recs.size() * sizeof(palace_fasta_rec)));
            for (; k < h_dup.size(); k++)
                if (h_dup[k])
                    std::fprintf(stderr, "make_fa_from_path: warning: %s: sequence name '%.*s' appears again in record %zu: the first one is used\n", fasta.c_str(),
                                 static_cast<int>(recs[k].name_len), text.data + recs[k].name_off, k + 1);
        }
        tr.lap("names hashed");
    }
};

struct Job { std::string paths, out, mode; };

// one paths file -> one FASTA.  The output file exists (empty) from the start; nothing is written to it before every token is resolved
void run_job(palace_ctx *ctx, const std::string &fasta, std::unique_ptr<Assembly> &assembly, const Job &job, palace_host::Trace &tr)
{
    std::fputs("make_fa_from_path.py running\n", stdout);
    if (!assembly) assembly = std::make_unique<Assembly>(ctx, fasta, tr);
    const Assembly &as = *assembly;
    palace_host::MappedText ptext;
    try { ptext.open(job.paths); }
    catch (const std::exception &) { throw Failure("cannot open " + job.paths); }
    std::FILE *out = std::fopen(job.out.c_str(), "wb");
    if (!out) throw Failure("cannot write " + job.out);
    palace_host::FileGuard closer{out};
    const palace_host::PathTokens tk = palace_host::split_paths(ptext.data, ptext.size);
    const int64_t n_tok = static_cast<int64_t>(tk.tokens()), n_paths = static_cast<int64_t>(tk.lines());
    tr.lap("paths split");

    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const uint8_t *d_tok = dev.upload(reinterpret_cast<const uint8_t *>(tk.clean.data()), tk.clean.size(), "the tokens");
    const int64_t *d_tok_off = dev.upload(tk.clean_off.data(), tk.clean_off.size(), "the tokens' offsets");
    int32_t *d_code = dev.array<int32_t>(static_cast<size_t>(n_tok), "the tokens' records");
    HIP_OK(palace_path_resolve(ctx, as.names.h, d_tok, d_tok_off, n_tok, d_code));
    std::vector<int32_t> code(static_cast<size_t>(n_tok));
    if (n_tok) HIP_OK(palace_d2h(ctx, code.data(), d_code, code.size() * sizeof(int32_t)));
    for (int64_t l = 0; l < n_paths; l++)
        for (int64_t t = tk.line_tok[static_cast<size_t>(l)]; t < tk.line_tok[static_cast<size_t>(l) + 1]; t++) {
            const int32_t c = code[static_cast<size_t>(t)];
            if (c == PALACE_PATH_NOTHING) continue;
            const std::string token = tk.clean.substr(static_cast<size_t>(tk.clean_off[static_cast<size_t>(t)]),
                                                      static_cast<size_t>(tk.clean_off[static_cast<size_t>(t) + 1] - tk.clean_off[static_cast<size_t>(t)]));
            const bool oriented = token.back() == '+' || token.back() == '-';
            if (!oriented && (c == PALACE_PATH_NOT_FOUND || (c & PALACE_PATH_SECOND_TRY))) {
                const size_t cut = token.rfind('_');
                std::printf("Contig not found: %s\n", cut == std::string::npos ? "" : token.substr(0, cut).c_str());
            }
            if (c == PALACE_PATH_NOT_FOUND) {
                std::fflush(stdout);
                throw Failure(job.paths + ": line " + std::to_string(tk.line_index[static_cast<size_t>(l)] + 1) + ": contig of token '" + token +
                              "' is not in " + fasta);
            }
        }
    tr.lap("tokens resolved");

    const int64_t *d_path_off = dev.upload(tk.line_tok.data(), tk.line_tok.size(), "the paths' tokens");
    int64_t *d_cum = dev.array<int64_t>(static_cast<size_t>(n_tok + 1), "the tokens' places");
    int64_t *d_len = dev.array<int64_t>(static_cast<size_t>(n_paths), "the paths' lengths");
    HIP_OK(palace_path_fasta_lengths(ctx, as.d_recs, d_code, n_tok, d_path_off, n_paths, d_cum, d_len));
    std::vector<int64_t> len(static_cast<size_t>(n_paths));
    if (n_paths) HIP_OK(palace_d2h(ctx, len.data(), d_len, len.size() * sizeof(int64_t)));
    std::string hdr;
    std::vector<int64_t> hdr_off{0}, path_out{0};
    for (int64_t l = 0; l < n_paths; l++) {
        if (job.mode == "0") hdr += "res_" + std::to_string(tk.line_index[static_cast<size_t>(l)] + 1) + "_" + std::to_string(len[static_cast<size_t>(l)]);
        else hdr.append(tk.raw, static_cast<size_t>(tk.raw_off[static_cast<size_t>(tk.line_tok[static_cast<size_t>(l)])]),
                        static_cast<size_t>(tk.raw_off[static_cast<size_t>(tk.line_tok[static_cast<size_t>(l) + 1])] - tk.raw_off[static_cast<size_t>(tk.line_tok[static_cast<size_t>(l)])]));
        path_out.push_back(path_out.back() + (static_cast<int64_t>(hdr.size()) - hdr_off.back()) + len[static_cast<size_t>(l)] + 3);
        hdr_off.push_back(static_cast<int64_t>(hdr.size()));
    }
    const int64_t total = path_out.back();
    const uint8_t *d_hdr = dev.upload(reinterpret_cast<const uint8_t *>(hdr.data()), hdr.size(), "the headers");
    const int64_t *d_hdr_off = dev.upload(hdr_off.data(), hdr_off.size(), "the headers' offsets");
    const int64_t *d_path_out = dev.upload(path_out.data(), path_out.size(), "the paths' places");
    tr.lap("lengths and headers");

    if (total) {                                                             // the output text, in windows (output_windows.hpp)
        palace_host::WindowWriter windows(ctx, dev, "PALACE_PATHFA_WINDOW", total);
        windows.write(total, out, job.out, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_path_fasta_write(ctx, as.d_text, as.d_recs, d_code, d_cum, d_path_off, n_paths, d_hdr, d_hdr_off, d_path_out, lo, hi, d_win));
        });
    }
    closer.release();
    if (std::fclose(out) != 0) throw Failure("cannot write " + job.out);
    tr.lap("output written");
}

}  // namespace

int main(int argc, char **argv)
{
    std::vector<Job> jobs;
    std::string fasta, list;
    if (argc == 5 && std::string(argv[1]) != "--batch") { fasta = argv[1]; jobs.push_back(Job{argv[2], argv[3], argv[4]}); }
    else if (argc == 4 && std::string(argv[1]) == "--batch") { list = argv[2]; fasta = argv[3]; }
    else {
        std::fputs("Usage: make_fa_from_path <fasta_file> <paths_file> <output_file> <mode>\n"
                   "       make_fa_from_path --batch <list of '<paths_file> <output_file> <mode>' lines> <fasta_file>\n", stderr);
        return 1;
    }
    palace_host::FastExit fast_exit = palace_host::fast_exit_begin();   // from here on this is the worker process (fast_exit.hpp)
    const int device = palace_host::pick_device();                       // PALACE_DEVICE (device_pick.hpp): before anything touches HIP
    palace_host::Trace tr("make_fa_from_path");
    palace_ctx *ctx = nullptr;
    if (palace_ctx_create(device, &ctx) != PALACE_OK) {
        std::fprintf(stderr, "make_fa_from_path: no GPU device to work on (%s); there is no CPU path\n", palace_last_error());
        return 1;
    }
    tr.lap("device up");
    try {
        if (!list.empty()) {
            std::ifstream lf(list);
            if (!lf) throw Failure("cannot open batch list " + list);
            for (std::string line; std::getline(lf, line);) {
                std::vector<palace_host::sv> t;
                palace_host::split_ws(line, t);
                if (t.empty()) continue;
                if (t.size() != 3) throw Failure("batch list: expected '<paths> <out.fasta> <mode>' per line");
                jobs.push_back(Job{std::string(t[0]), std::string(t[1]), std::string(t[2])});
            }
        }
        std::unique_ptr<Assembly> assembly;
        for (const Job &j : jobs) run_job(ctx, fasta, assembly, j, tr);
    } catch (const std::exception &e) {
        std::fflush(stdout);
        std::fprintf(stderr, "make_fa_from_path: %s\n", e.what());
        return 1;
    }
    fast_exit.done(0);          // outputs are complete and closed: the caller goes on, the teardown happens behind it
}
