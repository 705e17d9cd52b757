// The header's contig names on the device, for whoever looks a name up there (bam.hip: the SA items' contigs; sam.hip: RNAME and
// RNEXT): the table palace_bam_names_create builds, and the probe.
#pragma once
#include "name_hash.hpp"

// the blob and offsets are the caller's, the table is this object's.  slots[k] = a tid or -1;
// equal names share one slot that holds the largest tid (the last duplicate wins, as BamColumns::tid_of)
struct palace_bam_names {
    const uint8_t *names;
    const int64_t *off;
    int32_t n_ref;
    uint32_t mask;
    int32_t *slots;
};

namespace palace {

__device__ __forceinline__ bool is_name(const palace_bam_names &t, int32_t tid, const uint8_t *p, int64_t n)
{
    return same_bytes(t.names + t.off[tid], t.off[tid + 1] - t.off[tid], p, n);
}

// linear probing without removals: a name sits between its hash's slot and the first empty one (the table is at most half full)
__device__ __forceinline__ int32_t tid_of(const palace_bam_names &t, const uint8_t *p, int64_t n)
{
    for (uint32_t at = hash_name(p, n) & t.mask;; at = (at + 1) & t.mask) {
        const int32_t tid = t.slots[at];
        if (tid < 0) return -1;
        if (is_name(t, tid, p, n)) return tid;
    }
}

}  // namespace palace
