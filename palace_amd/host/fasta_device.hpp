// A FASTA text that lies on the device: its index and the table of its names (csrc/path_fasta.hip), as make_fa_from_path,
// make_final_fa and split_fastg ask for them.  What a fault of the text or a name that appears twice means is the tool's.
#pragma once
#include <vector>

#include "device_scope.hpp"

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

}  // namespace palace_host
