// What the text writers (path_fasta.hip, fastg_split.hip) share: the second and third launch of a 64-bit exclusive scan whose first
// launch leaves per-block sums (kScanThreads entries per block), and the search of a place in such a scan.
#pragma once
#include "text_lanes.hpp"

namespace palace {
namespace {

constexpr int kScanThreads = 1024;

// one workgroup: sums[0 .. nb) become their exclusive prefix sums, sums[nb] the total
__global__ __launch_bounds__(kScanThreads) void block_sums_scan_kernel(long long *sums, int64_t nb)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t per = (nb + kScanThreads - 1) / kScanThreads;
    const int64_t b0 = threadIdx.x * per < nb ? threadIdx.x * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    long long mine = 0, total;
    for (int64_t k = b0; k < b1; k++) mine += sums[k];
    long long run = block_exclusive<long long, kScanThreads>(mine, s_scan, &total);
    for (int64_t k = b0; k < b1; k++) { const long long v = sums[k]; sums[k] = run; run += v; }
    if (threadIdx.x == 0) sums[nb] = total;
}

// cum[i] becomes the scan's entry (its block's base added), cum[n] the total
__global__ __launch_bounds__(kScanThreads) void add_block_base_kernel(int64_t n, int64_t *cum, const long long *block_base, int64_t nb)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    if (i < n) cum[i] += block_base[blockIdx.x];
    if (i == 0) cum[n] = block_base[nb];
}

// the last index in [a, b] whose entry is <= v (v >= arr[a])
__device__ __forceinline__ int64_t last_le(const int64_t *arr, int64_t a, int64_t b, int64_t v)
{
    while (a < b) {
        const int64_t mid = a + (b - a + 1) / 2;
        if (arr[mid] <= v) a = mid; else b = mid - 1;
    }
    return a;
}

}  // namespace
}  // namespace palace
