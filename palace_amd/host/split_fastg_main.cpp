// split_fastg -g <assembly_graph.fastg> [-o <nodes.fasta>] [--fai]: the reference's share/palace/scripts/split_fastg.py (call
// site palace:389-397) with its command line, the FASTG indexed, its records named and the FASTA gathered on the device
// (csrc/fastg_split.hip; the rules: DESIGN.md 8).  The host reads the file, asks for the verdict and writes what comes back; no
// name is derived and no base is turned here.
//   --fai: also <output>.fai and <graph>.fai, the rows of the three `samtools faidx` runs behind the script (palace:399-406),
//   written as decimal text on the device.  In <graph>.fai a record whose whole name an earlier record has is left out, with one
//   warning line on stderr.
// The FASTG, the output and the tables have to fit the device: there is no path around it.  Exit 0 with nothing on stdout; 1
// for a text outside the grammar (the message names the smallest line at fault; the output file is left empty) or any other
// failure; 2 for a usage error.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
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

// the FASTG's own faults on top of the FASTA index's
const char *fault_text(int code)
{
    switch (code) {
    case PALACE_FASTG_EPLUS: return "a sequence line that begins with '+' or '@'";
    case PALACE_FASTG_EHIGH: return "a byte of 0x80 or above in a header line";
    case PALACE_FASTG_ECR: return "a CR in a header line that is not directly before the LF";
    case PALACE_FASTG_ENOLF: return "the text does not end in LF";
    case PALACE_FASTG_EEMPTY: return "the file is empty";
    case PALACE_FASTG_ENONAME: return "a header without a name in front of its last byte, its first ':' or ','";
    case PALACE_FASTG_EBASE: return "a base other than A, C, G, T in a primed record";
    }
    return palace_host::fasta_fault_text(code);
}

void run(palace_ctx *ctx, const std::string &graph, const std::string &output, bool fai, palace_host::Trace &tr)
{
    palace_host::MappedText text;
    palace_host::open_text(text, graph);
    palace_host::PendingOutputs outputs;
    std::FILE *out = outputs.open(output, true);                             // (exists, empty, from here on: as the script's)
    tr.lap("FASTG read");
    const int64_t n = static_cast<int64_t>(text.size);
    DeviceScope dev(ctx, palace_host::no_room_does_not_fit);
    const uint8_t *d_text = dev.upload(text.bytes(), text.size, "the FASTG is read on the device and has no other path: it");
    tr.lap("FASTG uploaded");

    const palace_host::FastaIndex ix = palace_host::index_fasta(ctx, dev, d_text, n, "the FASTG's index");
    palace_fasta_status st = ix.st, fg{};
    palace_fasta_rec *const d_recs = ix.d_recs;
    const int64_t n_records = st.n_records;
    const size_t nr = static_cast<size_t>(n_records);
    tr.lap("FASTG indexed");
    palace_fasta_rec *d_name_recs = dev.array<palace_fasta_rec>(nr, "the records' names");
    uint8_t *d_primed = dev.array<uint8_t>(nr, "the primed bits");
    HIP_OK(palace_fastg_derive(ctx, d_text, n, d_recs, n_records, d_name_recs, d_primed, &fg));
    tr.lap("names derived, text checked");
    if (fg.error && (!st.error || fg.bad_line < st.bad_line || (fg.bad_line == st.bad_line && fg.error < st.error))) st = fg;
    if (st.error) palace_host::line_fault(graph, st.bad_line, fault_text(st.error));

    palace_host::FastaNamesHandle names(ctx);
    uint8_t *d_dup = dev.array<uint8_t>(nr, "the duplicate flags");
    HIP_OK(palace_fasta_names_create(ctx, d_text, d_name_recs, n_records, d_dup, &names.h));
    int64_t *d_out_off = dev.array<int64_t>(nr + 1, "the records' places");
    palace_fasta_rec *d_out_recs = dev.array<palace_fasta_rec>(fai ? nr : 0, "the output's index");
    int64_t n_kept = 0, total = 0;
    HIP_OK(palace_fastg_plan(ctx, d_name_recs, d_dup, n_records, d_out_off, fai ? d_out_recs : nullptr, &n_kept, &total));
    tr.lap("names hashed, output planned");
    uint8_t *d_out = dev.array<uint8_t>(static_cast<size_t>(total), "the output is gathered on the device and has no other path: it");
    HIP_OK(palace_fastg_write(ctx, d_text, d_name_recs, d_primed, d_out_off, n_records, 0, total, d_out));
    HIP_OK(palace_sync(ctx));
    tr.lap("output gathered");
    palace_host::device_to_file(ctx, d_out, total, out, output);
    dev.give_back(d_out);
    if (!outputs.commit()) throw Failure("cannot write " + output);
    tr.lap("output written");
    if (!fai) return;

    palace_host::write_fai(ctx, d_text, d_out_recs, d_dup, n_records, output + ".fai", true);
    palace_host::FastaNamesHandle whole(ctx);
    uint8_t *d_skip = dev.array<uint8_t>(nr, "the duplicate flags");
    HIP_OK(palace_fasta_names_create(ctx, d_text, d_recs, n_records, d_skip, &whole.h));
    palace_host::write_fai(ctx, d_text, d_recs, d_skip, n_records, graph + ".fai", true);
    std::vector<uint8_t> skip(nr);
    if (n_records) HIP_OK(palace_d2h(ctx, skip.data(), d_skip, skip.size()));
    palace_host::for_each_duplicate(ctx, skip, d_recs, text.data, [&](size_t k, const palace_fasta_rec &r, const char *t) {
        std::fprintf(stderr, "split_fastg: warning: %s: sequence name '%.*s' appears again in record %zu: left out of %s.fai\n", graph.c_str(),
                     static_cast<int>(r.name_len), t + r.name_off, k + 1, graph.c_str());
    });
    tr.lap("index rows written");
}

int usage(const char *why)
{
    std::fprintf(stderr, "usage: split_fastg [-h] -g GRAPH [-o OUTPUT] [--fai]\nsplit_fastg: error: %s\n", why);
    return 2;
}

// the script's default: X.fastg -> X.nodes.fasta (what os.path.splitext makes of the name); "" for any other name, whose default
// would be the graph itself
std::string default_output(const std::string &graph)
{
    const size_t slash = graph.rfind('/');
    size_t base = slash == std::string::npos ? 0 : slash + 1;
    while (base < graph.size() && graph[base] == '.') base++;                // leading dots belong to the root
    const std::string ext = ".fastg", rest = graph.substr(base);
    if (rest.size() <= ext.size() || rest.compare(rest.size() - ext.size(), ext.size(), ext) != 0) return "";
    return graph.substr(0, graph.size() - ext.size()) + ".nodes.fasta";
}

}  // namespace

int main(int argc, char **argv)
{
    std::string graph, output;
    bool have_graph = false, have_output = false, fai = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const std::string &shrt, const std::string &lng, std::string *into, bool *have) -> int {      // 1 taken, 0 not this option, -1 no value
            if (a == shrt || a == lng) {
                if (i + 1 >= argc) return -1;
                *into = argv[++i]; *have = true;
                return 1;
            }
            for (const std::string &o : {shrt, lng})
                if (a.compare(0, o.size() + 1, o + "=") == 0) { *into = a.substr(o.size() + 1); *have = true; return 1; }
            return 0;
        };
        if (a == "--fai") { fai = true; continue; }
        int r = value("-g", "--graph", &graph, &have_graph);
        if (r == 0) r = value("-o", "--output", &output, &have_output);
        if (r < 0) return usage(("argument " + a + ": expected one argument").c_str());
        if (r == 0) return usage(("unrecognized arguments: " + a).c_str());
    }
    if (!have_graph) return usage("the following arguments are required: -g/--graph");
    if (!have_output || output.empty()) {                                    // (the script takes an empty -o for none)
        output = default_output(graph);
        if (output.empty()) return usage("without -o the graph has to be named X.fastg (the output is then X.nodes.fasta)");
    }
    return palace_host::device_tool("split_fastg", [&](palace_ctx *ctx, palace_host::Trace &tr) { run(ctx, graph, output, fai, tr); });
}
