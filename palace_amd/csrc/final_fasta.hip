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
// The writer is path_fasta.hip's with three differences: a token's place in its path's sequence includes the separator in front
// of it (palace_final_fasta_lengths decides that: separator iff bytes were accumulated before), a path without bytes has no text
// at all, and a reversed record is complemented by the ambiguous-DNA table.
#include "common.hpp"
#include "scan64.hpp"
#include "text_lanes.hpp"

#include <climits>

namespace palace {
namespace {

constexpr int kTrimThreads = 256, kTrimWaves = kTrimThreads / 64;
constexpr int kTileThreads = 256, kTileBytes = kTileThreads * kLaneBytes;

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

__global__ __launch_bounds__(kScanThreads) void final_tok_scan_kernel(const palace_fasta_rec *recs, const int32_t *code, int64_t n_tok, const int64_t *path_off,
                                                                      int64_t n_paths, const unsigned long long *first_nz, int64_t sep_len, int64_t *cum,
                                                                      long long *block_sum)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    long long v = 0;
    if (i < n_tok && is_found(code[i]))
        v = recs[code[i] >> 2].length + (static_cast<unsigned long long>(i) > first_nz[last_le(path_off, 0, n_paths - 1, i)] ? sep_len : 0);
    long long total;
    const long long ex = block_exclusive<long long, kScanThreads>(v, s_scan, &total);
    if (i < n_tok) cum[i] = ex;
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void final_path_len_kernel(const int64_t *cum, const int64_t *path_off, int64_t n_paths, int64_t *len)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p < n_paths) len[p] = cum[path_off[p + 1]] - cum[path_off[p]];
}

// ---- the writer -------------------------------------------------------------------------------------------------------------------

// Biopython's ambiguous-DNA complement as the XOR of a letter's low five bits: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H; S, W, N
// and every other byte stay.  The same in either case.
__constant__ uint8_t kCompXor[32] = {
    0,
    'A' ^ 'T', 'B' ^ 'V', 'C' ^ 'G', 'D' ^ 'H', 0, 0, 'G' ^ 'C', 'H' ^ 'D', 0, 0, 'K' ^ 'M', 0, 'M' ^ 'K',   // A .. M
    0, 0, 0, 0, 'R' ^ 'Y', 0, 'T' ^ 'A', 0, 'V' ^ 'B', 0, 0, 'Y' ^ 'R', 0,                                   // N .. Z
    0, 0, 0, 0, 0};
__device__ __forceinline__ uint32_t complement(uint32_t b)
{
    return (b & 0xc0u) == 0x40u ? b ^ kCompXor[b & 0x1fu] : b;
}
__device__ __forceinline__ uint32_t complement4(uint32_t w)
{
    return complement(w & 0xffu) | (complement((w >> 8) & 0xffu) << 8) | (complement((w >> 16) & 0xffu) << 16) | (complement(w >> 24) << 24);
}

__global__ __launch_bounds__(kTileThreads) void final_write_kernel(const uint8_t *text, const palace_fasta_rec *recs, const int32_t *code, const int64_t *cum,
                                                                   const int64_t *path_off, int64_t n_paths, const uint8_t *hdr, const int64_t *hdr_off,
                                                                   const int64_t *path_out, uint32_t sep_byte, int64_t lo, int64_t hi, uint8_t *out)
{
    __shared__ long long s_path[2];
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTileBytes;
    if (threadIdx.x < 2) {                                                   // the paths of the tile's first and last byte
        const int64_t end = lo + tile0 + kTileBytes < hi ? lo + tile0 + kTileBytes : hi;
        s_path[threadIdx.x] = last_le(path_out, 0, n_paths - 1, threadIdx.x == 0 ? lo + tile0 : end - 1);
    }
    __syncthreads();
    const int64_t j0 = tile0 + threadIdx.x * kLaneBytes, o0 = lo + j0;
    if (o0 >= hi) return;
    const int cnt = hi - o0 < kLaneBytes ? static_cast<int>(hi - o0) : kLaneBytes;
    int64_t p = last_le(path_out, s_path[0], s_path[1], o0);                 // (the last of equal entries: a path with text)
    uint64_t acc_lo = 0, acc_hi = 0;
    int k = 0;
    auto put = [&](uint32_t b) {
        if (k < 8) acc_lo |= static_cast<uint64_t>(b) << (8 * k); else acc_hi |= static_cast<uint64_t>(b) << (8 * (k - 8));
        k++;
    };
    while (k < cnt) {
        const int64_t h0 = hdr_off[p], h = hdr_off[p + 1] - h0, ta = path_off[p], tb = path_off[p + 1], base = cum[ta], len = cum[tb] - base;
        int64_t x = o0 + k - path_out[p];                                    // the byte's place in the path's text
        for (; k < cnt && x < h + 2; x++) put(x == 0 ? '>' : x == h + 1 ? '\n' : hdr[h0 + x - 1]);
        if (k >= cnt) break;
        int64_t q = x - (h + 2);                                             // ... in its sequence
        if (q < len) {
            int64_t t = last_le(cum, ta, tb - 1, base + q);                  // (behind tokens without bytes it is the last of equal entries)
            while (k < cnt && q < len) {
                while (cum[t + 1] <= base + q) t++;
                const int32_t c = code[t];
                const palace_fasta_rec r = recs[c >> 2];
                const int64_t sep = cum[t + 1] - cum[t] - r.length, u = base + q - cum[t];     // the separator's bytes come first
                if (u < sep) {
                    const int64_t left = sep - u;
                    const int m = left < cnt - k ? static_cast<int>(left) : cnt - k;
                    for (int i = 0; i < m; i++) put(sep_byte);
                    q += m;
                    continue;
                }
                const int64_t left = cum[t + 1] - base - q;
                const int m = left < cnt - k ? static_cast<int>(left) : cnt - k;
                const bool rev = (c & PALACE_PATH_REVERSE) != 0;
                int64_t pos = u - sep;
                if (rev) pos = r.length - 1 - pos;
                const int64_t row = pos / r.line_bases;
                int64_t col = pos - row * r.line_bases, src = r.seq_off + row * r.line_width + col;
                if (m == kLaneBytes && (rev ? col >= kLaneBytes - 1 : col + kLaneBytes <= r.line_bases)) {
                    // the lane's 16 bytes are 16 neighbours of one line: one load, one store
                    uint4 v;
                    __builtin_memcpy(&v, text + (rev ? src - (kLaneBytes - 1) : src), sizeof v);
                    if (rev)
                        v = make_uint4(__builtin_bswap32(complement4(v.w)), __builtin_bswap32(complement4(v.z)), __builtin_bswap32(complement4(v.y)),
                                       __builtin_bswap32(complement4(v.x)));
                    *reinterpret_cast<uint4 *>(out + j0) = v;
                    return;
                }
                const int64_t gap = r.line_width - r.line_bases;
                for (int i = 0; i < m; i++) {
                    const uint32_t b = text[src];
                    put(rev ? complement(b) : b);
                    if (rev) { if (col == 0) { col = r.line_bases - 1; src -= gap + 1; } else { col--; src--; } }
                    else if (++col == r.line_bases) { col = 0; src += gap + 1; } else src++;
                }
                q += m;
            }
            if (k >= cnt) break;
        }
        put('\n');                                                           // the sequence's LF: the path is done
        do p++; while (p < n_paths - 1 && path_out[p + 1] == path_out[p]);   // (paths without text are passed over)
    }
    if (cnt == kLaneBytes)
        *reinterpret_cast<uint4 *>(out + j0) = make_uint4(static_cast<uint32_t>(acc_lo), static_cast<uint32_t>(acc_lo >> 32), static_cast<uint32_t>(acc_hi),
                                                          static_cast<uint32_t>(acc_hi >> 32));
    else
        for (int i = 0; i < cnt; i++) out[j0 + i] = static_cast<uint8_t>((i < 8 ? acc_lo >> (8 * i) : acc_hi >> (8 * (i - 8))) & 0xffu);
}

inline size_t align256(size_t b) { return (b + 255) & ~static_cast<size_t>(255); }

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
    const int64_t nb = (n_tok + kScanThreads - 1) / kScanThreads;
    if (nb == 0) PALACE_HIP_TRY(hipMemsetAsync(d_tok_cum, 0, sizeof(int64_t), ctx->stream));
    else {
        const size_t b_first = align256(static_cast<size_t>(n_paths) * sizeof(unsigned long long));
        const int rc = ensure_workspace(ctx, b_first + static_cast<size_t>(nb + 1) * sizeof(long long));
        if (rc) return rc;
        unsigned long long *first_nz = static_cast<unsigned long long *>(ctx->ws.ptr);
        long long *sums = reinterpret_cast<long long *>(static_cast<uint8_t *>(ctx->ws.ptr) + b_first);
        PALACE_HIP_TRY(hipMemsetAsync(first_nz, 0xff, static_cast<size_t>(n_paths) * sizeof(unsigned long long), ctx->stream));       // every path: none
        hipLaunchKernelGGL(final_first_kernel, dim3(static_cast<unsigned>((n_tok + 255) / 256)), dim3(256), 0, ctx->stream, d_recs, d_code, n_tok, d_path_off,
                           n_paths, first_nz);
        hipLaunchKernelGGL(final_tok_scan_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, d_recs, d_code, n_tok, d_path_off, n_paths,
                           first_nz, sep_len, d_tok_cum, sums);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
        hipLaunchKernelGGL(add_block_base_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n_tok, d_tok_cum, sums, nb);
    }
    if (n_paths)
        hipLaunchKernelGGL(final_path_len_kernel, dim3(static_cast<unsigned>((n_paths + 255) / 256)), dim3(256), 0, ctx->stream, d_tok_cum, d_path_off, n_paths,
                           d_path_len);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_final_fasta_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code,
                                        const int64_t *d_tok_cum, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr,
                                        const int64_t *d_hdr_off, const int64_t *d_path_out, int32_t sep_byte, int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && lo >= 0 && lo <= hi && sep_byte >= 0 && sep_byte <= 255, "bad argument");
    if (lo == hi) return PALACE_OK;
    PALACE_REQUIRE(n_paths > 0 && d_tok_cum && d_path_off && d_hdr_off && d_path_out && d_out, "null device pointer (or bytes asked of an empty text)");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (hi - lo + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE(nt < (1ll << 31), "window too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(final_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, d_recs, d_code, d_tok_cum, d_path_off,
                       n_paths, d_hdr, d_hdr_off, d_path_out, static_cast<uint32_t>(sep_byte), lo, hi, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
