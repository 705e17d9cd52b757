// corrected_dup's device half (include/palace_hip.h: palace_path_borders .. palace_paths_base_set_in; the rules: DESIGN.md 8): what
// the reference's corrected_dup.py does that is quadratic or worse in a path's length or in the number of paths, as integer problems
// over the tokens' ids, their lengths and their bases' ids.  Nothing here knows a name or a depth.
//
// Borders.  A workgroup owns a path, a wave a border length i (from n / 2 downwards, four at a time), its lanes stride the i
// comparisons of tok[0 .. i) with tok[n - i .. n); a wave whose compare holds raises the workgroup's maximum in LDS, and a wave
// whose i is no longer above that maximum stops.  A maximum does not depend on who raised it first.
//
// Tandem candidates.  A workgroup owns a path and loops over the periods r.  For one period a lane owns a position q and forms
// eq[q] = (tok[q] == tok[q + r]); R(s), the ones from s on, is a segmented suffix scan over eq: the positions are walked from the
// last 256 to the first, a wave's 64 flags are one ballot, a lane counts the ones above it in its wave's word, goes on through the
// words of the waves above it (LDS) while they are full, and ends in the run that the chunk above left at its first position (one
// word of LDS).  A path of equal tokens therefore costs what any other path of its length costs: n / 2 periods of n / 256 steps,
// no table of n x n entries, no loop over a run.  The candidates of a period are counted in one such pass and -- fill call only --
// placed in a second one from the period's end backwards, so that they stand in ascending s although the walk descends.
//
// The paths' distinct sorted values.  One stable palace_sort_u64 of path << 32 | value keeps every path's tokens in the path's own
// range and puts equal values next to each other; a flag where a key differs from the one before it, a scan of the flags
// (scan64.hpp), and the flagged values scattered by ordinal are the paths' distinct values, ascending, back to back; path p's begin
// at the scan's entry of its first token.  The similarity relation uses them as sets of lengths: S a wave's sum, I a search of the
// shorter set's values in the longer, the verdict 10 I >= 9 S (DESIGN.md 8 states why that is the rule's IEEE division).  The
// base-set test uses them as canonical lists: a 64-bit sum of mixed (value, place) words per path, the cycles' sums sorted, and a
// later path looks its own sum up, then compares value by value with every cycle of that sum -- a collision costs compares, never
// the result.
#include "common.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"     // (scan64.hpp's last_le is used by one kernel only)
#include "scan64.hpp"
#pragma clang diagnostic pop

namespace palace {
namespace {

constexpr int kPathThreads = 256, kPathWaves = kPathThreads / kWave;
constexpr int kMaxTandemPath = 1 << 20;
constexpr uint64_t kMaxLengthSum = 1ull << 49;

static_assert(PALACE_PATHS_REL_NONE == 0 && PALACE_PATHS_REL_J_LOSES == 1 && PALACE_PATHS_REL_I_LOSES == 2, "the header states the codes");

// ---- borders ---------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kPathThreads) void path_borders_kernel(const int32_t *node, const int64_t *off, int32_t *border)
{
    __shared__ int s_best;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = off[blockIdx.x];
    const int n = static_cast<int>(off[blockIdx.x + 1] - b);
    const int32_t *tok = node + b;
    if (threadIdx.x == 0) s_best = 0;
    __syncthreads();
    for (int i = n / 2 - wave; i >= 1; i -= kPathWaves) {                    // (uniform in the wave; no workgroup barrier inside)
        if (i <= *static_cast<volatile int *>(&s_best)) break;
        bool same = true;
        for (int k = lane; k < i && same; k += kWave) same = tok[k] == tok[n - i + k];
        if (__all(same)) {
            if (lane == 0) atomicMax(&s_best, i);
            break;                                                           // (every later i of this wave is smaller)
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) border[blockIdx.x] = s_best;
}

// ---- tandem candidates -----------------------------------------------------------------------------------------------------------------

struct TandemLds {
    unsigned long long mask[2][kPathWaves];    // eq of the waves' 64 positions, this step's and the one before
    int cnt[2][kPathWaves];                    // the waves' candidates
    int carry[2];                              // R at the chunk's first position
};

__device__ __forceinline__ int ones_from_bit0(unsigned long long m)
{
    const unsigned long long inv = ~m;
    return inv ? __ffsll(inv) - 1 : 64;
}

// One pass over the positions of period r, from the last chunk down: returns the period's candidates (the same in every lane).
// kFill: cand_end is the end of the period's entries, and every candidate writes its own, counted from there backwards.
template <bool kFill>
__device__ __forceinline__ long long tandem_pass(const int32_t *tok, int n, int r, TandemLds &L, int32_t *cand_end)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = n - r, last_start = n - 2 * r;
    const int chunks = (m + kPathThreads - 1) / kPathThreads;
    long long taken = 0;
    int it = 0;
    for (int k = chunks - 1; k >= 0; k--, it ^= 1) {
        const int q = k * kPathThreads + static_cast<int>(threadIdx.x);
        const bool eq = q < m && tok[q] == tok[q + r];
        const unsigned long long M = __ballot(eq);
        if (lane == 0) L.mask[it][wave] = M;
        __syncthreads();
        int run = ones_from_bit0(M >> lane);                                 // (the bits a shift brings in are zeros: at most 64 - lane)
        bool open = run == 64 - lane;
        for (int w = wave + 1; open && w < kPathWaves; w++) {
            const int t = ones_from_bit0(L.mask[it][w]);
            run += t;
            open = t == 64;
        }
        if (open && k != chunks - 1) run += L.carry[it ^ 1];
        if (threadIdx.x == 0) L.carry[it] = run;
        const bool cand = q <= last_start && run >= r;
        const unsigned long long CM = __ballot(cand);
        if (lane == 0) L.cnt[it][wave] = __popcll(CM);
        __syncthreads();
        int above = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kPathWaves; w++) {
            const int c = L.cnt[it][w];
            all += c;
            if (w > wave) above += c;
        }
        if (kFill && cand) {
            above += __popcll((CM >> lane) >> 1);
            int32_t *o = cand_end - 3 * (taken + above + 1);
            o[0] = r;
            o[1] = q;
            o[2] = 1 + run / r;
        }
        taken += all;
    }
    __syncthreads();                                                         // (the next pass begins with slot 0 again)
    return taken;
}

template <bool kFill>
__global__ __launch_bounds__(kPathThreads) void path_tandems_kernel(const int32_t *node, const int64_t *off, long long *count, const int64_t *cand_off, int32_t *cand,
                                                                    unsigned long long *err)
{
    __shared__ TandemLds L;
    const int64_t p = blockIdx.x, b = off[p], len = off[p + 1] - b;
    if (len >= kMaxTandemPath) {                                             // (uniform in the workgroup)
        if (threadIdx.x == 0) {
            atomicMin(err, static_cast<unsigned long long>(p));
            if (!kFill) count[p] = 0;
        }
        return;
    }
    const int n = static_cast<int>(len);
    const int32_t *tok = node + b;
    int32_t *out = kFill ? cand + 3 * cand_off[p] : nullptr;
    long long total = 0;
    for (int r = 1; r <= n / 2; r++) {
        const long long c = tandem_pass<false>(tok, n, r, L, nullptr);
        if (kFill && c) tandem_pass<true>(tok, n, r, L, out + 3 * (total + c));
        total += c;
    }
    if (!kFill && threadIdx.x == 0) count[p] = total;
}

struct CountSize {
    const long long *count;
    __device__ long long operator()(int64_t i) const { return count[i]; }
};

// ---- the paths' distinct sorted values ----------------------------------------------------------------------------------------------

// key[t] = path << 32 | value; Value reads token t's value (0 .. 2^32 - 1) or reports the token
template <class Value>
__global__ __launch_bounds__(256) void path_value_keys_kernel(Value value, int64_t n_tok, const int64_t *off, int64_t n_paths, uint64_t *key, unsigned long long *err)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const int64_t v = value(t);
    if (v < 0 || v > 0xffffffffll) { atomicMin(err, static_cast<unsigned long long>(t)); key[t] = 0; return; }
    const int64_t p = last_le(off, 0, n_paths - 1, t);
    key[t] = (static_cast<uint64_t>(p) << 32) | static_cast<uint64_t>(v);
}
struct LengthValue {
    const int64_t *len;
    __device__ int64_t operator()(int64_t t) const { return len[t]; }
};
struct BaseValue {
    const int32_t *base;
    __device__ int64_t operator()(int64_t t) const { return base[t]; }
};

struct HeadSize {
    const uint64_t *key;
    __device__ long long operator()(int64_t i) const { return i == 0 || key[i] != key[i - 1]; }
};

__global__ __launch_bounds__(256) void distinct_scatter_kernel(const uint64_t *key, const int64_t *cum, int64_t n_tok, uint32_t *val)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t < n_tok && cum[t + 1] != cum[t]) val[cum[t]] = static_cast<uint32_t>(key[t]);
}

// dstart[p], p = 0 .. n_paths: where path p's distinct values begin (the sort kept every path's tokens in the path's own range)
__global__ __launch_bounds__(256) void distinct_starts_kernel(const int64_t *cum, const int64_t *off, int64_t n_paths, int64_t *dstart)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p <= n_paths) dstart[p] = cum ? cum[off[p]] : 0;
}

// The distinct values of every path in the workspace from byte `at` on: val (n_tok uint32), dstart (n_paths + 1 int64).  `extra`
// bytes behind them are the caller's.
struct Distinct {
    uint32_t *val;
    int64_t *dstart;
    uint8_t *extra;
};

template <class Value>
int distinct_values(palace_ctx *ctx, const char *who, Value value, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, int32_t path_bits, size_t extra,
                    Distinct *out)
{
    const size_t n = static_cast<size_t>(n_tok), sort_bytes = palace_sort_u64_scratch_bytes(n_tok);
    const size_t b_val = align256(n * 4 + 4), b_start = align256((static_cast<size_t>(n_paths) + 1) * 8), b_extra = align256(extra), b_key = align256(n * 8 + 8),
                 b_perm = align256(n * 4 + 4), b_cum = align256((n + 1) * 8), b_sort = align256(sort_bytes), b_sums = align256(scan_sizes_bytes(n_tok));
    const int rc = ensure_workspace(ctx, b_val + b_start + b_extra + b_key + b_perm + b_cum + b_sort + b_sums);
    if (rc) return rc;
    uint8_t *w = static_cast<uint8_t *>(ctx->ws.ptr);
    out->val = reinterpret_cast<uint32_t *>(w);
    out->dstart = reinterpret_cast<int64_t *>(w + b_val);
    out->extra = w + b_val + b_start;
    uint8_t *t = out->extra + b_extra;
    uint64_t *key = reinterpret_cast<uint64_t *>(t);
    uint32_t *perm = reinterpret_cast<uint32_t *>(t + b_key);
    int64_t *cum = reinterpret_cast<int64_t *>(t + b_key + b_perm);
    void *sort_scratch = t + b_key + b_perm + b_cum;
    long long *sums = reinterpret_cast<long long *>(t + b_key + b_perm + b_cum + b_sort);
    const dim3 paths(static_cast<unsigned>((n_paths + 256) / 256));
    if (n_tok == 0) {
        hipLaunchKernelGGL(distinct_starts_kernel, paths, dim3(256), 0, ctx->stream, static_cast<const int64_t *>(nullptr), d_path_off, n_paths, out->dstart);
        PALACE_HIP_TRY(hipGetLastError());
        return PALACE_OK;
    }
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small), bad = ~0ull;
    PALACE_HIP_TRY(hipMemcpyAsync(small, &bad, sizeof bad, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (bad is this call's own)
    const dim3 toks(static_cast<unsigned>((n_tok + 255) / 256));
    hipLaunchKernelGGL(path_value_keys_kernel<Value>, toks, dim3(256), 0, ctx->stream, value, n_tok, d_path_off, n_paths, key, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(&bad, small, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (bad != ~0ull) {
        set_error("%s: token %llu has a value outside 0 .. 2^32 - 1", who, bad);
        return PALACE_EINVAL;
    }
    const int src = palace_sort_u64(ctx, key, perm, n_tok, 32 + path_bits, sort_scratch, sort_bytes);
    if (src) return src;
    scan_sizes_into(ctx, HeadSize{key}, n_tok, cum, sums);
    hipLaunchKernelGGL(distinct_scatter_kernel, toks, dim3(256), 0, ctx->stream, key, cum, n_tok, out->val);
    hipLaunchKernelGGL(distinct_starts_kernel, paths, dim3(256), 0, ctx->stream, cum, d_path_off, n_paths, out->dstart);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

int32_t bits_of(int64_t n)                                                   // the bits of the numbers below n
{
    int32_t b = 0;
    while (b < 31 && (1ll << b) < n) b++;
    return b;
}

// ---- the similarity relation -----------------------------------------------------------------------------------------------------------

// a wave owns a path: S = the sum of its distinct lengths; the greatest of them all goes to *max_sum
__global__ __launch_bounds__(kPathThreads) void length_sums_kernel(const uint32_t *val, const int64_t *dstart, int64_t n_paths, uint64_t *sum, unsigned long long *max_sum)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kPathWaves + wave;
    if (p >= n_paths) return;
    uint64_t s = 0;
    for (int64_t k = dstart[p] + lane; k < dstart[p + 1]; k += kWave) s += val[k];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) {
        sum[p] = s;
        atomicMax(max_sum, static_cast<unsigned long long>(s));
    }
}

__device__ __forceinline__ uint32_t pair_relation(const uint32_t *val, const int64_t *dstart, const uint64_t *sum, int64_t i, int64_t j)
{
    int64_t a0 = dstart[i], a1 = dstart[i + 1], b0 = dstart[j], b1 = dstart[j + 1];
    if (a1 - a0 > b1 - b0) { int64_t t = a0; a0 = b0; b0 = t; t = a1; a1 = b1; b1 = t; }
    uint64_t inter = 0;
    for (int64_t k = a0; k < a1; k++) {
        const uint32_t v = val[k];
        int64_t lo = b0, hi = b1;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (val[mid] < v) lo = mid + 1; else hi = mid;
        }
        if (lo < b1 && val[lo] == v) inter += v;
    }
    const uint64_t si = sum[i], sj = sum[j];
    if (10 * inter >= 9 * si || 10 * inter >= 9 * sj) return si > sj ? PALACE_PATHS_REL_J_LOSES : PALACE_PATHS_REL_I_LOSES;
    return PALACE_PATHS_REL_NONE;
}

// a lane owns a byte of the relation: the four pairs 4 k .. 4 k + 3 of the n_paths x n_paths table
__global__ __launch_bounds__(256) void length_relation_kernel(const uint32_t *val, const int64_t *dstart, const uint64_t *sum, int64_t n_paths, int64_t n_bytes, uint8_t *rel)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n_bytes) return;
    uint32_t byte = 0;
    for (int e = 0; e < 4; e++) {
        const int64_t idx = 4 * k + e, i = idx / n_paths, j = idx % n_paths;
        if (i < n_paths && i < j) byte |= pair_relation(val, dstart, sum, i, j) << (2 * e);
    }
    rel[k] = static_cast<uint8_t>(byte);
}

// ---- the base-set test -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// a wave owns a path: the sum over its canonical list of mixed (value, place) words, cut to the mask
__global__ __launch_bounds__(kPathThreads) void set_hash_kernel(const uint32_t *val, const int64_t *dstart, int64_t n_paths, uint64_t mask, uint64_t *hash)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kPathWaves + wave;
    if (p >= n_paths) return;
    const int64_t a = dstart[p];
    uint64_t s = 0;
    for (int64_t k = a + lane; k < dstart[p + 1]; k += kWave) s += mix64((static_cast<uint64_t>(k - a) << 32) | val[k]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) hash[p] = mix64(s + static_cast<uint64_t>(dstart[p + 1] - a)) & mask;
}

__global__ __launch_bounds__(256) void copy_keys_kernel(const uint64_t *src, int64_t n, uint64_t *dst)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k < n) dst[k] = src[k];
}

// a lane owns a path: 0 for a cycle; a later path finds the first cycle key that is not below its own and walks the equal ones
__global__ __launch_bounds__(256) void set_in_kernel(const uint32_t *val, const int64_t *dstart, const uint64_t *hash, const uint64_t *ckey, const uint32_t *cperm,
                                                     int64_t n_cycles, int64_t n_paths, uint8_t *in)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n_paths) return;
    uint8_t found = 0;
    if (p >= n_cycles) {
        const uint64_t h = hash[p];
        const int64_t a = dstart[p], len = dstart[p + 1] - a;
        int64_t lo = 0, hi = n_cycles;
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (ckey[mid] < h) lo = mid + 1; else hi = mid;
        }
        for (; lo < n_cycles && ckey[lo] == h && !found; lo++) {
            const int64_t c = cperm[lo], ca = dstart[c];
            if (dstart[c + 1] - ca != len) continue;
            bool same = true;
            for (int64_t k = 0; k < len && same; k++) same = val[a + k] == val[ca + k];
            found = same;
        }
    }
    in[p] = found;
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_path_borders(palace_ctx *ctx, const int32_t *d_node, const int64_t *d_path_off, int64_t n_paths, int32_t *d_border)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && n_paths < (1ll << 31), "bad argument (paths < 2^31)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_border, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(path_borders_kernel, dim3(static_cast<unsigned>(n_paths)), dim3(kPathThreads), 0, ctx->stream, d_node, d_path_off, d_border);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_path_tandems(palace_ctx *ctx, const int32_t *d_node, const int64_t *d_path_off, int64_t n_paths, int64_t *d_cand_off, int32_t *d_cand,
                                   int64_t cap, int64_t *n_cand_out)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && n_paths < (1ll << 31) && cap >= 0 && n_cand_out, "bad argument (paths < 2^31)");
    *n_cand_out = 0;
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_cand_off, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t b_count = align256(static_cast<size_t>(n_paths) * 8);
    const int rc = ensure_workspace(ctx, b_count + scan_sizes_bytes(n_paths));
    if (rc) return rc;
    uint8_t *w = static_cast<uint8_t *>(ctx->ws.ptr);
    long long *count = reinterpret_cast<long long *>(w);
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small), bad = ~0ull;
    PALACE_HIP_TRY(hipMemcpyAsync(small, &bad, sizeof bad, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (bad is this call's own)
    const dim3 grid(static_cast<unsigned>(n_paths));
    hipLaunchKernelGGL(path_tandems_kernel<false>, grid, dim3(kPathThreads), 0, ctx->stream, d_node, d_path_off, count, static_cast<const int64_t *>(nullptr),
                       static_cast<int32_t *>(nullptr), small);
    PALACE_HIP_TRY(hipGetLastError());
    scan_sizes_into(ctx, CountSize{count}, n_paths, d_cand_off, reinterpret_cast<long long *>(w + b_count));
    PALACE_HIP_TRY(hipGetLastError());
    long long total = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&bad, small, sizeof bad, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(&total, d_cand_off + n_paths, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (bad != ~0ull) {
        set_error("palace_path_tandems: path %llu has 2^20 tokens or more", bad);
        return PALACE_EINVAL;
    }
    *n_cand_out = total;
    if (!d_cand) return PALACE_OK;
    PALACE_REQUIRE(cap >= total, "cap is smaller than the number of candidates");
    if (total == 0) return PALACE_OK;
    hipLaunchKernelGGL(path_tandems_kernel<true>, grid, dim3(kPathThreads), 0, ctx->stream, d_node, d_path_off, static_cast<long long *>(nullptr), d_cand_off, d_cand,
                       small);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" size_t palace_paths_length_relation_bytes(int64_t n_paths)
{
    return n_paths > 0 ? static_cast<size_t>((n_paths * n_paths + 3) / 4) : 0;
}

extern "C" int palace_paths_length_relation(palace_ctx *ctx, const int64_t *d_len, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, uint8_t *d_rel)
{
    PALACE_REQUIRE(ctx && n_tok >= 0 && n_tok < (1ll << 31) && n_paths >= 0 && n_paths < (1ll << 15), "bad argument (tokens < 2^31, paths < 2^15)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_rel && (d_len || n_tok == 0), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    Distinct d;
    const int rc = distinct_values(ctx, __func__, LengthValue{d_len}, n_tok, d_path_off, n_paths, bits_of(n_paths), static_cast<size_t>(n_paths) * 8, &d);
    if (rc) return rc;
    uint64_t *sum = reinterpret_cast<uint64_t *>(d.extra);
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small), max_sum = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(small, &max_sum, sizeof max_sum, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (max_sum is this call's own)
    hipLaunchKernelGGL(length_sums_kernel, dim3(static_cast<unsigned>((n_paths + kPathWaves - 1) / kPathWaves)), dim3(kPathThreads), 0, ctx->stream, d.val, d.dstart,
                       n_paths, sum, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(&max_sum, small, sizeof max_sum, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    PALACE_REQUIRE(max_sum < kMaxLengthSum, "a path's distinct lengths sum to 2^49 or more");
    const int64_t n_bytes = static_cast<int64_t>(palace_paths_length_relation_bytes(n_paths));
    hipLaunchKernelGGL(length_relation_kernel, dim3(static_cast<unsigned>((n_bytes + 255) / 256)), dim3(256), 0, ctx->stream, d.val, d.dstart, sum, n_paths, n_bytes,
                       d_rel);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_paths_base_set_in(palace_ctx *ctx, const int32_t *d_base, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, int64_t n_cycles,
                                        int32_t hash_bits, uint8_t *d_in)
{
    PALACE_REQUIRE(ctx && n_tok >= 0 && n_tok < (1ll << 31) && n_paths >= 0 && n_paths < (1ll << 31) && n_cycles >= 0 && n_cycles <= n_paths && hash_bits >= 0 &&
                       hash_bits <= 64,
                   "bad argument (tokens, paths < 2^31, cycles <= paths, hash_bits 0 .. 64)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_in && (d_base || n_tok == 0), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t np = static_cast<size_t>(n_paths), nc = static_cast<size_t>(n_cycles), sort_bytes = palace_sort_u64_scratch_bytes(n_cycles);
    const size_t b_hash = align256(np * 8), b_ckey = align256(nc * 8 + 8), b_cperm = align256(nc * 4 + 4);
    Distinct d;
    const int rc = distinct_values(ctx, __func__, BaseValue{d_base}, n_tok, d_path_off, n_paths, bits_of(n_paths), b_hash + b_ckey + b_cperm + align256(sort_bytes), &d);
    if (rc) return rc;
    uint64_t *hash = reinterpret_cast<uint64_t *>(d.extra), *ckey = reinterpret_cast<uint64_t *>(d.extra + b_hash);
    uint32_t *cperm = reinterpret_cast<uint32_t *>(d.extra + b_hash + b_ckey);
    void *sort_scratch = d.extra + b_hash + b_ckey + b_cperm;
    const uint64_t mask = hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    hipLaunchKernelGGL(set_hash_kernel, dim3(static_cast<unsigned>((n_paths + kPathWaves - 1) / kPathWaves)), dim3(kPathThreads), 0, ctx->stream, d.val, d.dstart, n_paths,
                       mask, hash);
    PALACE_HIP_TRY(hipGetLastError());
    if (n_cycles) {
        hipLaunchKernelGGL(copy_keys_kernel, dim3(static_cast<unsigned>((n_cycles + 255) / 256)), dim3(256), 0, ctx->stream, hash, n_cycles, ckey);
        PALACE_HIP_TRY(hipGetLastError());
        const int src = palace_sort_u64(ctx, ckey, cperm, n_cycles, hash_bits, sort_scratch, sort_bytes);
        if (src) return src;
    }
    hipLaunchKernelGGL(set_in_kernel, dim3(static_cast<unsigned>((n_paths + 255) / 256)), dim3(256), 0, ctx->stream, d.val, d.dstart, hash, ckey, cperm, n_cycles, n_paths,
                       d_in);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
