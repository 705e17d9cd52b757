// The 64-bit exclusive scan of per-item sizes into places, and the search of a place in such a scan.  Three launches: per-block
// scans that leave block sums (kScanThreads entries per block), one workgroup over the sums, the bases added.  scan_sizes is all
// three for sizes stated as a functor (paths_writer.hpp, final_fasta.hip, fastg_split.hip, contig_features.hip); bam_sort.hip,
// bam_index.hip, sam.hip and readqc.hip bring a first launch of their own -- two scans at once, or a scan fused with other work --
// and use the second and third from here.  last_le is what the writers of window_lanes.hpp find an output byte's item with.
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

template <class Size>
__global__ __launch_bounds__(kScanThreads) void size_scan_kernel(Size size, int64_t n, int64_t *cum, long long *block_sum)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    const long long v = i < n ? size(i) : 0;
    long long total;
    const long long ex = block_exclusive<long long, kScanThreads>(v, s_scan, &total);
    if (i < n) cum[i] = ex;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// the bytes of block sums a scan of n sizes needs
inline size_t scan_sizes_bytes(int64_t n) { return static_cast<size_t>((n + kScanThreads - 1) / kScanThreads + 1) * sizeof(long long); }

// cum[0 .. n]: the exclusive prefix sums of size(0 .. n) and their total (n > 0); sums: scan_sizes_bytes(n) bytes of the caller's
template <class Size>
void scan_sizes_into(palace_ctx *ctx, Size size, int64_t n, int64_t *cum, long long *sums)
{
    const int64_t nb = (n + kScanThreads - 1) / kScanThreads;
    hipLaunchKernelGGL(size_scan_kernel<Size>, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, size, n, cum, sums);
    hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(add_block_base_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n, cum, sums, nb);
}

// The same with the block sums in the context's workspace, from byte ws_at on (a multiple of 8).  A caller that keeps something of
// its own in front of them -- what `size` reads, say -- asks for ws_at + scan_sizes_bytes(n) itself before it takes a pointer: the
// workspace is then large enough and does not move here.
template <class Size>
int scan_sizes(palace_ctx *ctx, Size size, int64_t n, int64_t *cum, size_t ws_at = 0)
{
    const int rc = ensure_workspace(ctx, ws_at + scan_sizes_bytes(n));
    if (rc) return rc;
    scan_sizes_into(ctx, size, n, cum, reinterpret_cast<long long *>(static_cast<uint8_t *>(ctx->ws.ptr) + ws_at));
    return PALACE_OK;
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
