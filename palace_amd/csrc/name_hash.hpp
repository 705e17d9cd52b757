// What the device's name tables share (bam.hip: the BAM header's contigs; path_fasta.hip: the records of a FASTA): the hash of a
// name's bytes and the byte compare behind a probe.  Which of two equal names a table keeps is each table's own rule.
#pragma once
#include "common.hpp"

namespace palace {

__device__ __forceinline__ uint32_t hash_name(const uint8_t *p, int64_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (int64_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return static_cast<uint32_t>(h);
}
__device__ __forceinline__ bool same_bytes(const uint8_t *a, int64_t na, const uint8_t *b, int64_t nb)
{
    if (na != nb) return false;
    for (int64_t i = 0; i < na; i++)
        if (a[i] != b[i]) return false;
    return true;
}

}  // namespace palace
