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
#include "fasta_device.hpp"
#include "fastx.hpp"
#include "output_windows.hpp"
#include "path_tokens.hpp"
#include "textio.hpp"
#include "trace.hpp"

namespace {

using palace_host::Failure;
using palace_host::DeviceScope;
using palace_host::Assembly;

struct Job { std::string paths, out, mode; };

// one paths file -> one FASTA.  The output file exists (empty) from the start; nothing is written to it before every token is resolved
void run_job(palace_ctx *ctx, const std::string &fasta, std::unique_ptr<Assembly> &assembly, const Job &job, palace_host::Trace &tr)
{
    std::fputs("make_fa_from_path.py running\n", stdout);
    if (!assembly) {
        assembly = std::make_unique<Assembly>(ctx, fasta);
        tr.lap("FASTA read");
        assembly->load(tr, [&](size_t k, const palace_fasta_rec &r, const char *text) {
            std::fprintf(stderr, "make_fa_from_path: warning: %s: sequence name '%.*s' appears again in record %zu: the first one is used\n", fasta.c_str(),
                         static_cast<int>(r.name_len), text + r.name_off, k + 1);
        });
    }
    const Assembly &as = *assembly;
    palace_host::MappedText ptext;
    palace_host::open_text(ptext, job.paths);
    palace_host::PendingOutputs outputs;
    std::FILE *out = outputs.open(job.out, true);
    const palace_host::PathTokens tk = palace_host::split_paths(ptext.data, ptext.size);
    const int64_t n_tok = static_cast<int64_t>(tk.tokens()), n_paths = static_cast<int64_t>(tk.lines());
    tr.lap("paths split");

    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const palace_host::Resolved res = palace_host::resolve(ctx, dev, as.names.h, tk.clean, tk.clean_off, palace_host::kTokensWhat, true);
    const std::vector<int32_t> &code = res.code;
    int32_t *const d_code = res.d_code;
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
    palace_host::PathsText plan;
    for (int64_t l = 0; l < n_paths; l++) {
        const size_t t0 = static_cast<size_t>(tk.line_tok[static_cast<size_t>(l)]), t1 = static_cast<size_t>(tk.line_tok[static_cast<size_t>(l) + 1]);
        if (job.mode == "0") plan.add("res_" + std::to_string(tk.line_index[static_cast<size_t>(l)] + 1) + "_" + std::to_string(len[static_cast<size_t>(l)]), len[static_cast<size_t>(l)]);
        else plan.add(std::string_view(tk.raw).substr(static_cast<size_t>(tk.raw_off[t0]), static_cast<size_t>(tk.raw_off[t1] - tk.raw_off[t0])), len[static_cast<size_t>(l)]);
    }
    const palace_host::PathsText::OnDevice pd = plan.upload(dev);
    const int64_t total = pd.total;
    tr.lap("lengths and headers");

    if (total) {                                                             // the output text, in windows (output_windows.hpp)
        palace_host::WindowWriter windows(ctx, dev, "PALACE_PATHFA_WINDOW", total);
        windows.write(total, out, job.out, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
            HIP_OK(palace_path_fasta_write(ctx, as.d_text, as.d_recs, d_code, d_cum, d_path_off, n_paths, pd.d_hdr, pd.d_hdr_off, pd.d_path_out, lo, hi, d_win));
        });
    }
    if (!outputs.commit()) throw Failure("cannot write " + job.out);
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
    return palace_host::device_tool("make_fa_from_path", [&](palace_ctx *ctx, palace_host::Trace &tr) {
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
    });
}
