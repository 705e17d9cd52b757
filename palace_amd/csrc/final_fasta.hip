// The last step of the pipeline on the device (include/palace_hip.h: palace_cycle_trim .. palace_final_fasta_write): what the
// reference's make_final_fa.py decides and writes, as an integer problem over node ids and a gather (the rules: DESIGN.md 8).
//
// The cycle test of a path of L tokens asks, over all 0 <= i <= j < L, for the interval of least (trimmed, i, j) among those with
// trimmed = sum len[0 .. i) + sum len(j .. L) <= threshold, an arc path[j] -> path[i], and distinct bases of path[i .. j] that sum
// to the minimum at least.  Five steps, the sort apart:
//   1. prefix: a workgroup per path leaves P[0 .. L], the sums of its first k lengths;
//   2. keys, palace_sort_u64, prev: a stable sort of the tokens by base puts the tokens of one base and one path next to each
//      other in path order: prev[t] = the token before t of t's base in t's path, or -1;
//   3. decide: a workgroup per path.  P[i] <= threshold bounds i from above (searched once), P[j + 1] >= total - (threshold -
//      P[i]) bounds j from below (searched once per i).  A wave takes an i, its lanes 64 values of j at a time from i upwards:
//      the distinct-base sum of [i, j] is the running sum of len[k], k in [i, j], prev[k] < i -- a wave scan with a carry -- and a
//      lane whose j is a candidate and whose sum suffices looks its arc up by binary search.  The lanes keep their least key; a
//      reduction over the wave and the four waves leaves the path's.
//
// The writer is paths_writer.hpp's, under FinalPolicy (below): a token's bytes include the separator in front of it (FinalTokSize
// decides that: separator iff bytes were accumulated before), a path without bytes has no text at all, and a reversed record is
// complemented by the ambiguous-DNA table.
#include "common.hpp"
#include "paths_writer.hpp"

#include <climits>

namespace palace {
namespace {

constexpr int kTrimThreads = 256, kTrimWaves = kTrimThreads / 64;

// ---- the cycle test ---------------------------------------------------------------------------------------------------------------

// path p's sums go to pre[path_off[p] + p .. path_off[p + 1] + p]: L + 1 entries per path, the first 0, the last the path's total
__global__ __launch_bounds__(kTrimThreads) void trim_prefix_kernel(const int64_t *len, const int64_t *path_off, int64_t *pre)
{
    __shared__ long long s_scan[kTrimWaves + 1];
    const int64_t p = blockIdx.x, a = path_off[p], L = path_off[p + 1] - a;
    int64_t *out = pre + a + p;
    long long carry = 0;
    for (int64_t k0 = 0; k0 < L; k0 += kTrimThreads) {                       // (uniform trip count)
        const int64_t k = k0 + threadIdx.x;
        const long long v = k < L ? len[a + k] : 0;
        long long total;
        const long long ex = block_exclusive<long long, kTrimThreads>(v, s_scan, &total);
        if (k < L) out[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) out[L] = carry;
}

__global__ __launch_bounds__(256) void trim_keys_kernel(const int32_t *base, int64_t n, uint64_t *key)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t < n) key[t] = static_cast<uint32_t>(base[t]);
}

// key / perm: the bases sorted, stably, so equal bases lie in token order and those of one path next to each other
__global__ __launch_bounds__(256) void trim_prev_kernel(const uint64_t *key, const uint32_t *perm, int64_t n, const int64_t *path_off, int64_t n_paths,
                                                        int32_t *prev)
{
    const int64_t s = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n) return;
    const uint32_t t = perm[s];
    int32_t pv = -1;
    if (s > 0 && key[s - 1] == key[s]) {
        const uint32_t u = perm[s - 1];                                      // (u < t)
        if (static_cast<int64_t>(u) >= path_off[last_le(path_off, 0, n_paths - 1, static_cast<int64_t>(t))]) pv = static_cast<int32_t>(u);
    }
    prev[t] = pv;
}

__device__ __forceinline__ bool has_arc(const uint64_t *arcs, int64_t n, uint64_t key)
{
    int64_t lo = 0, hi = n;                                                  // the first entry >= key
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (arcs[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && arcs[lo] == key;
}

__device__ __forceinline__ bool key_less(long long ta, unsigned long long ija, long long tb, unsigned long long ijb)
{
    return ta < tb || (ta == tb && ija < ijb);
}

__global__ __launch_bounds__(kTrimThreads) void cycle_trim_kernel(const int32_t *node, const int64_t *len, const int64_t *path_off, const int64_t *pre,
                                                                  const int32_t *prev, const uint64_t *arcs, int64_t n_arcs, int64_t thr, int64_t min_len,
                                                                  int32_t *first, int32_t *last)
{
    __shared__ long long s_t[kTrimWaves];
    __shared__ unsigned long long s_ij[kTrimWaves];
    const int64_t p = blockIdx.x, a = path_off[p], L = path_off[p + 1] - a;
    const int64_t *P = pre + a + p;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long best_t = LLONG_MAX;                                            // the key (trimmed, i << 32 | j); LLONG_MAX: none
    unsigned long long best_ij = ~0ull;
    if (L > 0 && thr >= 0 && n_arcs > 0) {
        const int64_t total = P[L];
        const int64_t imax = last_le(P, 0, L - 1, thr);                      // (P[0] = 0 <= thr)
        for (int64_t i = wave; i <= imax; i += kTrimWaves) {                 // (uniform in the wave; no workgroup barrier inside)
            const int64_t need = total - (thr - P[i]);                       // j is a candidate iff P[j + 1] >= need; j = L - 1 always is
            int64_t lo = i, hi = L - 1;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (P[mid + 1] >= need) hi = mid; else lo = mid + 1;
            }
            const int64_t jmin = lo;
            const uint32_t dst = static_cast<uint32_t>(node[a + i]);
            long long carry = 0;
            for (int64_t j0 = i; j0 < L; j0 += 64) {
                const int64_t j = j0 + lane;
                long long inc = (j < L && prev[a + j] < a + i) ? len[a + j] : 0;   // a base's first token at or behind i counts
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const long long o = __shfl_up(inc, d, 64);
                    if (lane >= d) inc += o;
                }
                const long long uniq = carry + inc;
                carry += __shfl(inc, 63, 64);
                if (j < L && j >= jmin && uniq >= min_len &&
                    has_arc(arcs, n_arcs, (static_cast<uint64_t>(static_cast<uint32_t>(node[a + j])) << 32) | dst)) {
                    const long long tr = P[i] + (total - P[j + 1]);
                    const unsigned long long ij = (static_cast<unsigned long long>(i) << 32) | static_cast<unsigned long long>(j);
                    if (key_less(tr, ij, best_t, best_ij)) { best_t = tr; best_ij = ij; }
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long ot = __shfl_xor(best_t, d, 64);
        const unsigned long long oij = __shfl_xor(best_ij, d, 64);
        if (key_less(ot, oij, best_t, best_ij)) { best_t = ot; best_ij = oij; }
    }
    if (lane == 0) { s_t[wave] = best_t; s_ij[wave] = best_ij; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kTrimWaves; w++)
            if (key_less(s_t[w], s_ij[w], best_t, best_ij)) { best_t = s_t[w]; best_ij = s_ij[w]; }
        const bool none = best_t == LLONG_MAX;
        first[p] = none ? -1 : static_cast<int32_t>(best_ij >> 32);
        last[p] = none ? -1 : static_cast<int32_t>(best_ij & 0xffffffffu);
    }
}

// ---- the tokens' places -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_found(int32_t c) { return c >= 0 && (c & PALACE_PATH_SECOND_TRY) == 0; }

// first_nz[p]: the first token of path p that brings bytes (~0: none): the tokens behind it are preceded by a separator
__global__ __launch_bounds__(256) void final_first_kernel(const palace_fasta_rec *recs, const int32_t *code, int64_t n_tok, const int64_t *path_off,
                                                          int64_t n_paths, unsigned long long *first_nz)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n_tok) return;
    const int32_t c = code[t];
    if (!is_found(c) || recs[c >> 2].length <= 0) return;
    atomicMin(&first_nz[last_le(path_off, 0, n_paths - 1, t)], static_cast<unsigned long long>(t));
}

// a token's bytes: its record's bases, and the separator in front of them behind its path's first token with bytes
struct FinalTokSize {
    const palace_fasta_rec *recs;
    const int32_t *code;
    const int64_t *path_off;
    int64_t n_paths;
    const unsigned long long *first_nz;
    int64_t sep_len;
    __device__ __forceinline__ long long operator()(int64_t t) const
    {
        if (!is_found(code[t])) return 0;
        return recs[code[t] >> 2].length + (static_cast<unsigned long long>(t) > first_nz[last_le(path_off, 0, n_paths - 1, t)] ? sep_len : 0);
    }
};

struct FinalPolicy {
    using Comp = ComplementAmbiguous;
    static constexpr bool kSeparator = true, kSkipEmptyPaths = true;
};

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_cycle_trim(palace_ctx *ctx, const int32_t *d_node, const int32_t *d_base, const int64_t *d_len, int64_t n_tok,
                                 const int64_t *d_path_off, int64_t n_paths, const uint64_t *d_arcs, int64_t n_arcs, int64_t trim_threshold,
                                 int64_t min_cycle_length, int32_t *d_first, int32_t *d_last)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && n_paths < (1ll << 31) && n_arcs >= 0 && n_tok >= 0 && n_tok < (1ll << 31), "bad argument (paths, tokens < 2^31)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_first && d_last && (n_tok == 0 || (d_node && d_base && d_len)) && (n_arcs == 0 || d_arcs), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    // the workspace: P, prev, and the sort's keys, permutation and scratch
    const size_t sort_bytes = palace_sort_u64_scratch_bytes(n_tok);
    const size_t b_pre = align256(static_cast<size_t>(n_tok + n_paths) * sizeof(int64_t)), b_prev = align256(static_cast<size_t>(n_tok) * sizeof(int32_t)),
                 b_key = align256(static_cast<size_t>(n_tok) * sizeof(uint64_t)), b_perm = align256(static_cast<size_t>(n_tok) * sizeof(uint32_t));
    const int rc = ensure_workspace(ctx, b_pre + b_prev + b_key + b_perm + sort_bytes + 256);
    if (rc) return rc;
    uint8_t *w = static_cast<uint8_t *>(ctx->ws.ptr);
    int64_t *pre = reinterpret_cast<int64_t *>(w);
    int32_t *prev = reinterpret_cast<int32_t *>(w + b_pre);
    uint64_t *key = reinterpret_cast<uint64_t *>(w + b_pre + b_prev);
    uint32_t *perm = reinterpret_cast<uint32_t *>(w + b_pre + b_prev + b_key);
    void *sort_scratch = w + b_pre + b_prev + b_key + b_perm;
    const dim3 paths(static_cast<unsigned>(n_paths));
    hipLaunchKernelGGL(trim_prefix_kernel, paths, dim3(kTrimThreads), 0, ctx->stream, d_len, d_path_off, pre);
    if (n_tok) {
        const dim3 toks(static_cast<unsigned>((n_tok + 255) / 256));
        hipLaunchKernelGGL(trim_keys_kernel, toks, dim3(256), 0, ctx->stream, d_base, n_tok, key);
        PALACE_HIP_TRY(hipGetLastError());
        const int src = palace_sort_u64(ctx, key, perm, n_tok, 32, sort_scratch, sort_bytes);
        if (src) return src;
        hipLaunchKernelGGL(trim_prev_kernel, toks, dim3(256), 0, ctx->stream, key, perm, n_tok, d_path_off, n_paths, prev);
    }
    hipLaunchKernelGGL(cycle_trim_kernel, paths, dim3(kTrimThreads), 0, ctx->stream, d_node, d_len, d_path_off, pre, prev, d_arcs, n_arcs, trim_threshold,
                       min_cycle_length, d_first, d_last);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_final_fasta_lengths(palace_ctx *ctx, const palace_fasta_rec *d_recs, const int32_t *d_code, int64_t n_tok, const int64_t *d_path_off,
                                          int64_t n_paths, int64_t sep_len, int64_t *d_tok_cum, int64_t *d_path_len)
{
    PALACE_REQUIRE(ctx && n_tok >= 0 && n_paths >= 0 && n_tok < (1ll << 39) && n_paths < (1ll << 39) && sep_len >= 0, "bad argument");
    PALACE_REQUIRE(d_tok_cum && d_path_off && (d_path_len || n_paths == 0) && (n_tok == 0 || (d_recs && d_code && n_paths > 0)), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    // the workspace: first_nz, and the scan's block sums behind it
    const size_t b_first = align256(static_cast<size_t>(n_paths) * sizeof(unsigned long long));
    unsigned long long *first_nz = nullptr;
    if (n_tok) {
        const int rc = ensure_workspace(ctx, b_first + scan_sizes_bytes(n_tok));
        if (rc) return rc;
        first_nz = static_cast<unsigned long long *>(ctx->ws.ptr);
        PALACE_HIP_TRY(hipMemsetAsync(first_nz, 0xff, static_cast<size_t>(n_paths) * sizeof(unsigned long long), ctx->stream));       // every path: none
        hipLaunchKernelGGL(final_first_kernel, dim3(static_cast<unsigned>((n_tok + 255) / 256)), dim3(256), 0, ctx->stream, d_recs, d_code, n_tok, d_path_off,
                           n_paths, first_nz);
    }
    return paths_lengths(ctx, FinalTokSize{d_recs, d_code, d_path_off, n_paths, first_nz, sep_len}, n_tok, d_path_off, n_paths, d_tok_cum, d_path_len, b_first);
}

extern "C" int palace_final_fasta_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code,
                                        const int64_t *d_tok_cum, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr,
                                        const int64_t *d_hdr_off, const int64_t *d_path_out, int32_t sep_byte, int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && lo >= 0 && lo <= hi && sep_byte >= 0 && sep_byte <= 255, "bad argument");
    return paths_write<FinalPolicy>(__func__, ctx, d_text, d_recs, d_code, d_tok_cum, d_path_off, n_paths, d_hdr, d_hdr_off, d_path_out,
                                    static_cast<uint32_t>(sep_byte), lo, hi, d_out);
}
