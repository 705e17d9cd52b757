// The table of a FASTA's record names as the kernels see it (palace_fasta_names_create builds it, path_fasta.hip): the look-up
// that palace_path_resolve and palace_blast_groups (filter_result.hip) share.
#pragma once
#include "name_hash.hpp"

struct palace_fasta_names {
    const uint8_t *text;
    const palace_fasta_rec *recs;
    int32_t n;
    uint32_t mask;
    int32_t *slots;                          // a record or -1; equal names share the slot, which holds the smallest record
};

namespace palace {

__device__ __forceinline__ bool is_name(const palace_fasta_names &t, int32_t r, const uint8_t *p, int64_t n)
{
    return same_bytes(t.text + t.recs[r].name_off, t.recs[r].name_len, p, n);
}

// the record of the name p[0 .. n), -1 when there is none: linear probing, the table never loses an entry
__device__ __forceinline__ int32_t record_of(const palace_fasta_names &t, const uint8_t *p, int64_t n)
{
    if (n <= 0) return -1;
    for (uint32_t at = hash_name(p, n) & t.mask;; at = (at + 1) & t.mask) {
        const int32_t r = t.slots[at];
        if (r < 0) return -1;
        if (is_name(t, r, p, n)) return r;
    }
}

}  // namespace palace
