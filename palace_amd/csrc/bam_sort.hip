// bamsort's sort half (the driver's `samtools sort`, palace:425-426) on the inflated stream where palace_bam_walk left
// it: one key per record (bam_record.hpp: sort_key), a stable LSD radix sort of the keys with the record ordinal as payload, the
// layout of the sorted stream (a 64-bit scan of the record sizes in sorted order) and the gather of the records' bytes.
//
// The sort.  A pass orders by one 8-bit digit; each pass is: every workgroup counts the digits of its tile of T = 4096 keys, one
// scan over the (digit, tile) counts, every workgroup ranks its tile again and scatters.  What makes a pass stable is the rank inside
// the tile: a wave owns 1024 consecutive keys and takes them 64 at a time; in a round the lanes of equal digit find each other
// with eight ballots, a lane's rank among them is the number of set bits below it, and the group's lowest lane adds the group to
// the wave's own 256 counters in LDS after every lane of the group has read the count so far.  The counters are private to a wave
// and a wave runs in lockstep, so there is no atomic and no bank conflict worth the name (random digits and LDS atomics are
// conflict bound here: DESIGN.md 9 item 1); the waves' counts are combined per digit by the workgroup's 256 lanes, one digit each.
#include "common.hpp"
#include "bam_record.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"     // (of scan64.hpp's three launches the last is done by gather_base_kernel here)
#include "scan64.hpp"
#pragma clang diagnostic pop

namespace palace {
namespace {

constexpr int kSortThreads = 256, kSortWaves = kSortThreads / kWave, kSortTile = PALACE_SORT_TILE;
constexpr int kWaveKeys = kSortTile / kSortWaves, kRounds = kWaveKeys / kWave;
static_assert(kSortThreads == 256, "one lane per digit combines the waves' counts");
static_assert(kRounds * kWave * kSortWaves == kSortTile, "a tile is whole rounds of whole waves");


// small[0] = records without a key, small[1] = the smallest ordinal among them
__global__ __launch_bounds__(256) void sort_keys_kernel(const uint8_t *stream, int64_t total, const int64_t *starts, int64_t n, int32_t n_ref,
                                                        uint64_t *key, unsigned long long *small)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s = starts[i];
    if (s < 4 || s + 32 > total || !sort_key_ok(stream, s, n_ref)) {
        atomicAdd(&small[0], 1ull);
        atomicMin(&small[1], static_cast<unsigned long long>(i));
        key[i] = ~0ull;
        return;
    }
    key[i] = sort_key(stream, s, n_ref);
}

// The tile's keys ranked by the digit (key >> shift) & mask: s_cnt[w][d] becomes the number of wave w's keys with digit d, and --
// when kRanks -- k[r] / rank[r] the key of the lane's round r and the number of keys of its digit in front of it in its wave.
template <bool kRanks>
__device__ __forceinline__ void rank_tile(const uint64_t *key, int64_t n, int shift, uint32_t mask, uint32_t (*s_cnt)[256], uint64_t *k, uint32_t *rank)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < kSortWaves * 256; d += kSortThreads) (&s_cnt[0][0])[d] = 0;
    __syncthreads();
    volatile uint32_t *cnt = s_cnt[wave];
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kSortTile + wave * kWaveKeys + lane;
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int64_t i = base + r * kWave;
        const bool valid = i < n;
        const uint64_t kk = valid ? key[i] : 0;
        const uint32_t dg = static_cast<uint32_t>(kk >> shift) & mask;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (dg >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t prev = valid ? cnt[dg] : 0;                           // every lane of a group reads the count so far ...
        __builtin_amdgcn_wave_barrier();
        if (valid && lane == __ffsll(static_cast<long long>(peers)) - 1) cnt[dg] = prev + static_cast<uint32_t>(__popcll(peers));   // ... then one adds the group
        __builtin_amdgcn_wave_barrier();
        if constexpr (kRanks) {
            k[r] = kk;
            rank[r] = prev + static_cast<uint32_t>(__popcll(peers & ((1ull << lane) - 1ull)));
        }
    }
    __syncthreads();
}

// hist[d * nb + tile] = keys of the tile with digit d
__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const uint64_t *key, int64_t n, int shift, uint32_t mask, uint32_t *hist, int64_t nb)
{
    __shared__ uint32_t s_cnt[kSortWaves][256];
    rank_tile<false>(key, n, shift, mask, s_cnt, nullptr, nullptr);
    const int d = threadIdx.x;
    uint32_t c = 0;
#pragma unroll
    for (int w = 0; w < kSortWaves; w++) c += s_cnt[w][d];
    hist[static_cast<int64_t>(d) * nb + blockIdx.x] = c;
}

// first launch of the scan over hist[0 .. m): exclusive sums inside blocks of kScanThreads entries, the blocks' sums for scan64.hpp
__global__ __launch_bounds__(kScanThreads) void sort_hist_scan_kernel(uint32_t *hist, int64_t m, long long *sums)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    const long long v = i < m ? hist[i] : 0;
    long long total;
    const long long ex = block_exclusive<long long, kScanThreads>(v, s_scan, &total);
    if (i < m) hist[i] = static_cast<uint32_t>(ex);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// perm_in null: the keys come in input order, the payload is the ordinal
__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const uint64_t *key_in, const uint32_t *perm_in, int64_t n, int shift, uint32_t mask,
                                                                    const uint32_t *hist, const long long *sums, int64_t nb, uint64_t *key_out,
                                                                    uint32_t *perm_out)
{
    __shared__ uint32_t s_cnt[kSortWaves][256];
    uint64_t k[kRounds];
    uint32_t rank[kRounds];
    rank_tile<true>(key_in, n, shift, mask, s_cnt, k, rank);
    {                                                                        // the place of each wave's first key of each digit
        const int d = threadIdx.x;
        const int64_t at = static_cast<int64_t>(d) * nb + blockIdx.x;
        uint32_t run = hist[at] + static_cast<uint32_t>(sums[at / kScanThreads]);
#pragma unroll
        for (int w = 0; w < kSortWaves; w++) { const uint32_t c = s_cnt[w][d]; s_cnt[w][d] = run; run += c; }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * kSortTile + wave * kWaveKeys + lane;
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int64_t i = base + r * kWave;
        if (i >= n) continue;
        const int64_t to = static_cast<int64_t>(s_cnt[wave][static_cast<uint32_t>(k[r] >> shift) & mask]) + rank[r];
        if (to >= n) continue;                                               // (cannot happen: the counts are those of these keys)
        key_out[to] = k[r];
        perm_out[to] = perm_in ? perm_in[i] : static_cast<uint32_t>(i);
    }
}

__global__ __launch_bounds__(256) void sort_iota_kernel(uint32_t *perm, int64_t n)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) perm[i] = static_cast<uint32_t>(i);
}

// ---- the sorted stream's layout and the gather --------------------------------------------------------------------------------

__global__ __launch_bounds__(kScanThreads) void gather_len_scan_kernel(const uint8_t *stream, const int64_t *starts, const uint32_t *perm, int64_t n,
                                                                       int64_t *cum, long long *sums)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    const long long v = i < n ? 4 + static_cast<long long>(ld32(stream, starts[perm[i]] - 4)) : 0;
    long long total;
    const long long ex = block_exclusive<long long, kScanThreads>(v, s_scan, &total);
    if (i < n) cum[i] = ex;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// cum[i] gets its block's base and the header's bytes, cum[n] the stream's length (block_base[nb] = all records' bytes)
__global__ __launch_bounds__(kScanThreads) void gather_base_kernel(int64_t n, int64_t head, int64_t *cum, const long long *block_base, int64_t nb,
                                                                   int64_t *starts_out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    if (i < n) {
        const int64_t v = cum[i] + block_base[blockIdx.x] + head;
        cum[i] = v;
        if (starts_out) starts_out[i] = v + 4;
    }
    if (i == 0) cum[n] = block_base[nb] + head;
}

constexpr int kGatherThreads = 256, kGatherTile = kGatherThreads * kLaneBytes;

__global__ __launch_bounds__(kGatherThreads) void gather_write_kernel(const uint8_t *stream, const int64_t *starts, const uint32_t *perm, const int64_t *off,
                                                                      int64_t n, uint8_t *out)
{
    __shared__ long long s_rec[2];
    const int64_t lo = off[0], hi = off[n];
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kGatherTile;
    if (threadIdx.x < 2) {                                                   // the records of the tile's first and last byte
        const int64_t a = tile0 > lo ? tile0 : lo, e = tile0 + kGatherTile < hi ? tile0 + kGatherTile : hi;
        s_rec[threadIdx.x] = a < e ? last_le(off, 0, n - 1, threadIdx.x == 0 ? a : e - 1) : 0;
    }
    __syncthreads();
    const int64_t j0 = tile0 + threadIdx.x * kLaneBytes;
    int64_t o = j0 > lo ? j0 : lo;
    const int64_t oe = j0 + kLaneBytes < hi ? j0 + kLaneBytes : hi;
    if (o >= oe) return;
    int64_t r = last_le(off, s_rec[0], s_rec[1], o);
    if (oe - o == kLaneBytes && off[r + 1] >= oe) {                          // the lane's 16 bytes are 16 neighbours of one record
        uint4 v;
        __builtin_memcpy(&v, stream + (starts[perm[r]] - 4 + (o - off[r])), sizeof v);
        *reinterpret_cast<uint4 *>(out + o) = v;
        return;
    }
    while (o < oe) {
        const int64_t src = starts[perm[r]] - 4 + (o - off[r]);
        const int64_t m = (off[r + 1] < oe ? off[r + 1] : oe) - o;
        for (int64_t q = 0; q < m; q++) out[o + q] = stream[src + q];
        o += m;
        r++;
    }
}

struct SortScratch { uint64_t *key; uint32_t *perm, *hist; long long *sums; int64_t nb, m, nblk; size_t bytes; };
SortScratch sort_scratch(int64_t n, void *base)
{
    SortScratch s;
    s.nb = (n + kSortTile - 1) / kSortTile;
    s.m = 256 * s.nb;
    s.nblk = (s.m + kScanThreads - 1) / kScanThreads;
    uint8_t *p = static_cast<uint8_t *>(base);
    size_t at = 0;
    s.key = reinterpret_cast<uint64_t *>(p + at); at += align256(static_cast<size_t>(n) * 8);
    s.perm = reinterpret_cast<uint32_t *>(p + at); at += align256(static_cast<size_t>(n) * 4);
    s.hist = reinterpret_cast<uint32_t *>(p + at); at += align256(static_cast<size_t>(s.m) * 4);
    s.sums = reinterpret_cast<long long *>(p + at); at += align256(static_cast<size_t>(s.nblk + 1) * 8);
    s.bytes = at;
    return s;
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_bam_sort_keys(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records, int32_t n_ref,
                                    uint64_t *d_key, int64_t *n_bad_out, int64_t *first_bad_out)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0 && n_ref >= 0 && n_bad_out && first_bad_out, "bad argument");
    PALACE_REQUIRE(n_records < (1ll << 31), "more than 2^31 - 1 records");
    PALACE_REQUIRE(n_records == 0 || (d_stream && d_starts && d_key), "null device pointer");
    *n_bad_out = 0;
    *first_bad_out = -1;
    if (n_records == 0) return PALACE_OK;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    const unsigned long long init[2] = {0, ~0ull};
    unsigned long long got[2];
    PALACE_HIP_TRY(hipMemcpyAsync(small, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (init is this call's own)
    hipLaunchKernelGGL(sort_keys_kernel, dim3(static_cast<unsigned>((n_records + 255) / 256)), dim3(256), 0, ctx->stream, d_stream, total, d_starts, n_records,
                       n_ref, d_key, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(got, small, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_bad_out = static_cast<int64_t>(got[0]);
    *first_bad_out = got[0] ? static_cast<int64_t>(got[1]) : -1;
    return PALACE_OK;
}

extern "C" size_t palace_sort_u64_scratch_bytes(int64_t n) { return n > 0 ? sort_scratch(n, nullptr).bytes : 0; }

extern "C" int palace_sort_u64(palace_ctx *ctx, uint64_t *d_key, uint32_t *d_perm, int64_t n, int32_t key_bits, void *d_scratch, size_t scratch_bytes)
{
    PALACE_REQUIRE(ctx && n >= 0 && n < (1ll << 31) && key_bits >= 0 && key_bits <= 64, "bad argument (n < 2^31, key_bits 0 .. 64)");
    if (n == 0) return PALACE_OK;
    PALACE_REQUIRE(d_key && d_perm && d_scratch, "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_scratch) & 255) == 0, "the scratch must be 256-byte aligned");
    PALACE_REQUIRE(scratch_bytes >= palace_sort_u64_scratch_bytes(n), "scratch smaller than palace_sort_u64_scratch_bytes(n)");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const SortScratch s = sort_scratch(n, d_scratch);
    const int passes = (key_bits + 7) / 8;
    if (passes == 0) {
        hipLaunchKernelGGL(sort_iota_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream, d_perm, n);
        PALACE_HIP_TRY(hipGetLastError());
        return PALACE_OK;
    }
    uint64_t *key[2] = {d_key, s.key};
    uint32_t *perm[2] = {d_perm, s.perm};
    const dim3 tiles(static_cast<unsigned>(s.nb));
    for (int p = 0; p < passes; p++) {
        const int shift = 8 * p, left = key_bits - shift;
        const uint32_t mask = left >= 8 ? 0xffu : (1u << left) - 1u;
        const int from = p & 1, to = from ^ 1;
        hipLaunchKernelGGL(sort_hist_kernel, tiles, dim3(kSortThreads), 0, ctx->stream, key[from], n, shift, mask, s.hist, s.nb);
        hipLaunchKernelGGL(sort_hist_scan_kernel, dim3(static_cast<unsigned>(s.nblk)), dim3(kScanThreads), 0, ctx->stream, s.hist, s.m, s.sums);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, s.sums, s.nblk);
        hipLaunchKernelGGL(sort_scatter_kernel, tiles, dim3(kSortThreads), 0, ctx->stream, key[from], p ? perm[from] : nullptr, n, shift, mask, s.hist, s.sums,
                           s.nb, key[to], perm[to]);
    }
    PALACE_HIP_TRY(hipGetLastError());
    if (passes & 1) {                                                        // the last pass wrote the scratch's pair
        PALACE_HIP_TRY(hipMemcpyAsync(d_key, s.key, static_cast<size_t>(n) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        PALACE_HIP_TRY(hipMemcpyAsync(d_perm, s.perm, static_cast<size_t>(n) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return PALACE_OK;
}

extern "C" int palace_bam_gather_plan(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const uint32_t *d_perm, int64_t n_records,
                                      int64_t head_bytes, int64_t *d_out_off, int64_t *d_out_starts, int64_t *out_bytes_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && head_bytes >= 0 && d_out_off && out_bytes_out, "bad argument");
    PALACE_REQUIRE(n_records == 0 || (d_stream && d_starts && d_perm), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nb = (n_records + kScanThreads - 1) / kScanThreads;
    const int rc = ensure_workspace(ctx, static_cast<size_t>(nb + 1) * sizeof(long long));
    if (rc) return rc;
    long long *sums = static_cast<long long *>(ctx->ws.ptr);
    if (nb == 0) PALACE_HIP_TRY(hipMemsetAsync(sums, 0, sizeof(long long), ctx->stream));
    else {
        hipLaunchKernelGGL(gather_len_scan_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, d_stream, d_starts, d_perm, n_records,
                           d_out_off, sums);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
    }
    hipLaunchKernelGGL(gather_base_kernel, dim3(static_cast<unsigned>(nb ? nb : 1)), dim3(kScanThreads), 0, ctx->stream, n_records, head_bytes, d_out_off, sums, nb,
                       d_out_starts);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(out_bytes_out, d_out_off + n_records, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PALACE_OK;
}

extern "C" int palace_bam_gather_write(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const uint32_t *d_perm, const int64_t *d_out_off,
                                       int64_t n_records, int64_t out_bytes, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && out_bytes >= 0, "bad argument");
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts && d_perm && d_out_off && d_out, "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (out_bytes + kGatherTile - 1) / kGatherTile;
    PALACE_REQUIRE(nt < (1ll << 31), "stream too long");
    if (nt == 0) return PALACE_OK;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(gather_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kGatherThreads), 0, ctx->stream, d_stream, d_starts, d_perm, d_out_off,
                       n_records, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
