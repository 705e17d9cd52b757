// A FASTA text that lies on the device: its index and the table of its names (csrc/path_fasta.hip).  `Assembly` is the whole of it
// for make_fa_from_path, make_final_fa and filter_result; split_fastg, whose names are derived first, takes index_fasta and
// for_each_duplicate; `resolve` turns names into records for the first three and for their ids_of / records_of.  What a name that
// appears twice means is the tool's.  `write_fai`: the index rows of a text to their file (split_fastg --fai, faidx).
#pragma once
#include <string>
#include <string_view>
#include <vector>

#include "device_scope.hpp"
#include "fastx.hpp"
#include "output_windows.hpp"
#include "trace.hpp"

namespace palace_host {

struct FastaIndex { palace_fasta_rec *d_recs; palace_fasta_status st; };

// the records of the text d_text[0 .. n): one call counts them, one fills them in.  The records are the scope's (named `what` where
// they do not fit); st.error says whether the text is one
inline FastaIndex index_fasta(palace_ctx *ctx, DeviceScope &dev, const uint8_t *d_text, int64_t n, const char *what)
{
    FastaIndex ix{nullptr, {}};
    const size_t sb = palace_fasta_index_scratch_bytes(n);
    void *d_scratch = dev.alloc(sb, "the index's scratch");
    HIP_OK(palace_fasta_index(ctx, d_text, n, nullptr, 0, d_scratch, sb, &ix.st));                                   // how many records
    ix.d_recs = dev.array<palace_fasta_rec>(static_cast<size_t>(ix.st.n_records), what);
    HIP_OK(palace_fasta_index(ctx, d_text, n, ix.d_recs, ix.st.n_records, d_scratch, sb, &ix.st));
    dev.give_back(d_scratch);
    return ix;
}

// the table of the records' names into `names`; returned, per record, whether an earlier record has its name
inline std::vector<uint8_t> hash_names(palace_ctx *ctx, DeviceScope &dev, const uint8_t *d_text, const palace_fasta_rec *d_recs, int64_t n_records,
                                       FastaNamesHandle &names)
{
    uint8_t *d_dup = dev.array<uint8_t>(static_cast<size_t>(n_records), "the duplicate flags");
    HIP_OK(palace_fasta_names_create(ctx, d_text, d_recs, n_records, d_dup, &names.h));
    std::vector<uint8_t> dup(static_cast<size_t>(n_records));
    if (n_records) HIP_OK(palace_d2h(ctx, dup.data(), d_dup, dup.size()));
    dev.give_back(d_dup);
    return dup;
}

// seen(k, record k, text) for every record k whose flag is set, in order.  (Rare: the records come to the host only to be named -- in
// one copy, and in none when no flag is set.)
template <class Seen>
void for_each_duplicate(palace_ctx *ctx, const std::vector<uint8_t> &dup, const palace_fasta_rec *d_recs, const char *text, Seen seen)
{
    size_t k = 0;
    for (; k < dup.size() && !dup[k]; k++) {}
    if (k == dup.size()) return;
    std::vector<palace_fasta_rec> recs(dup.size());
    HIP_OK(palace_d2h(ctx, recs.data(), d_recs, recs.size() * sizeof(palace_fasta_rec)));
    for (; k < dup.size(); k++)
        if (dup[k]) seen(k, recs[k], text);
}

// the `.fai` rows of d_recs (none where d_skip is set) to `path`: in place, or as `<path>.tmp` that gets its name when complete
inline void write_fai(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const uint8_t *d_skip, int64_t n_records, const std::string &path,
                      bool in_place)
{
    DeviceScope dev(ctx, no_room_does_not_fit);
    int64_t *d_off = dev.array<int64_t>(static_cast<size_t>(n_records + 1), "the rows' places");
    int64_t bytes = 0;
    HIP_OK(palace_fai_rows_plan(ctx, d_recs, d_skip, n_records, d_off, &bytes));
    uint8_t *d_rows = dev.array<uint8_t>(static_cast<size_t>(bytes), "the index rows");
    HIP_OK(palace_fai_rows_write(ctx, d_text, d_recs, d_skip, n_records, d_off, d_rows));
    PendingOutputs outputs;
    device_to_file(ctx, d_rows, bytes, outputs.open(path, in_place), path);
    if (!outputs.commit()) throw Failure("cannot write " + path);
}

// the 1-based line of the text that holds byte `at`
inline int64_t line_of(const char *text, int64_t at)
{
    int64_t line = 1;
    for (int64_t i = 0; i < at; i++) line += text[i] == '\n';
    return line;
}

// The assembly on the device: text, index, names.  Made, it is the mapped file (`cannot open <path>`); load() takes it to the device,
// faults where the text is no FASTA and hands every record whose name an earlier one has to duplicate(k, record, text).
struct Assembly {
    palace_ctx *ctx;
    std::string path;
    MappedText text;
    DeviceScope dev;
    FastaNamesHandle names;
    const uint8_t *d_text = nullptr;
    palace_fasta_rec *d_recs = nullptr;
    int64_t n_records = 0;

    Assembly(palace_ctx *c, const std::string &fasta) : ctx(c), path(fasta), dev(c, no_room_does_not_fit), names(c) { open_text(text, fasta); }

    template <class Duplicate> void load(Trace &tr, Duplicate duplicate)
    {
        d_text = dev.upload(text.bytes(), text.size, "the FASTA is read on the device and has no other path: it");
        tr.lap("FASTA uploaded");
        const FastaIndex ix = index_fasta(ctx, dev, d_text, static_cast<int64_t>(text.size), "the FASTA's index");
        if (ix.st.error) line_fault(path, ix.st.bad_line, fasta_fault_text(ix.st.error));
        d_recs = ix.d_recs;
        n_records = ix.st.n_records;
        tr.lap("FASTA indexed");
        for_each_duplicate(ctx, hash_names(ctx, dev, d_text, d_recs, n_records, names), d_recs, text.data, duplicate);
        tr.lap("names hashed");
    }
};

// Names -> records through a name table.  `text` holds n tokens one behind the other, token t being text[off[t] .. off[t + 1]); text,
// offsets and the n codes of palace_path_resolve go into `scope`, named as `what` says where they do not fit.  The codes stay on the
// device and come to the host as well when asked for.  names == nullptr: the table is made over the text itself, token `S+` being
// record t with the name S (ids_of of make_final_fa).
struct ResolveWhat { const char *text, *off, *code, *recs; };                // (recs: of the table over the text itself)
constexpr ResolveWhat kTokensWhat{"the tokens", "the tokens' offsets", "the tokens' records", nullptr};
struct Resolved { int32_t *d_code; std::vector<int32_t> code; };
inline Resolved resolve(palace_ctx *ctx, DeviceScope &scope, const palace_fasta_names *names, const std::string &text, const std::vector<int64_t> &off,
                        const ResolveWhat &what, bool to_host)
{
    const size_t n = off.size() - 1;
    const uint8_t *d_text = scope.upload(reinterpret_cast<const uint8_t *>(text.data()), text.size(), what.text);
    FastaNamesHandle own(ctx);
    if (!names) {
        std::vector<palace_fasta_rec> recs;
        for (size_t t = 0; t < n; t++) recs.push_back(palace_fasta_rec{off[t], off[t + 1] - off[t] - 1, 0, 0, 0, 0});
        const palace_fasta_rec *d_recs = scope.upload(recs.data(), recs.size(), what.recs);
        HIP_OK(palace_fasta_names_create(ctx, d_text, d_recs, static_cast<int64_t>(n), nullptr, &own.h));
        names = own.h;
    }
    const int64_t *d_off = scope.upload(off.data(), off.size(), what.off);
    Resolved r{scope.array<int32_t>(n, what.code), {}};
    HIP_OK(palace_path_resolve(ctx, names, d_text, d_off, static_cast<int64_t>(n), r.d_code));
    if (to_host) {
        r.code.resize(n);
        if (n) HIP_OK(palace_d2h(ctx, r.code.data(), r.d_code, n * sizeof(int32_t)));
    }
    return r;
}

// strings -> ids: one name table over the strings themselves, each followed by a '+' so that the bytes `S+` are at once record S
// of the table's text and the token palace_path_resolve takes the name S from.  The id of a string is its first record.
inline std::vector<int32_t> ids_of(palace_ctx *ctx, const std::vector<std::string_view> &strings)
{
    std::string text;
    std::vector<int64_t> off{0};
    for (const std::string_view s : strings) {
        text.append(s);
        text.push_back('+');
        off.push_back(static_cast<int64_t>(text.size()));
    }
    if (strings.empty()) return {};
    DeviceScope dev(ctx, no_room_does_not_fit);
    std::vector<int32_t> id = resolve(ctx, dev, nullptr, text, off, {"the node names", "the node names' offsets", "the node ids", "the node names' records"}, true).code;
    for (int32_t &c : id) {
        if (c < 0 || (c & 3)) throw Failure("internal: a node name did not resolve to itself");
        c >>= 2;
    }
    return id;
}

}  // namespace palace_host
