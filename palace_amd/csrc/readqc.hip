// readqc's device half (the driver's fastp call, palace:358-363): the records of a FASTQ text validated where the text lies
// (palace_fastq_records), every pair's overlap search, trim and filter decision with the scan of the output sizes (palace_readqc_plan),
// and the two output texts written in windows (palace_readqc_write).  What a record, a candidate and a filter MEAN is fastq_rules.hpp's;
// this file is who reads which byte.  The lines come from palace_sam_lines (sam.hip).
//
// A record.  A wavefront owns a record, four to a workgroup, as the lines of sam.hip: nothing is shared between them and no workgroup
// barrier is met.  Its lanes stride SEQ and QUAL 64 bytes at a time, a bad byte is one ballot.
//
// A pair.  A wavefront owns a pair and keeps A (read 1) and B (read 2 reversed and complemented) in LDS, 4096 bytes each: a candidate
// of the search reads up to 50 bytes of both at offsets only it knows, which registers cannot index.  The bases stay bytes: two bits a
// base would need a side channel for N and a shift per compared position, and the search is bound by the count of LDS reads, not by
// their width.  4 waves x 8 KiB = 32 KiB a workgroup: 5 workgroups of the CU's 160 KiB, 20 waves a CU, 5 of a SIMD's 8; the kernel's
// 100 VGPRs leave 4 of them.  The search is LDS reads back to back, which a few waves keep busy, so the missing ones cost little (at the
// 1M-contig sample the plan is 12 ms of a run of 0.7 s, profiles/readqc.md).  The candidates are taken 64 at a time in
// search order, a lane each; a lane leaves its candidate when it is over the limit and the wave leaves the round when all have; the first
// accepted one is the lowest bit of a ballot, and the round that has one is the last (the round count is the same for every lane).
// The filter's counts are ballots over the kept prefix.  The waves walk the pairs with a stride, so the eleven sums leave a wave
// once, not once per pair.
//
// The writer's lanes are window_lanes.hpp's: a lane owns 16 bytes of the window and stores them once; the items are the pairs, an
// item's text is the four lines of a read.
#include "common.hpp"
#include "fastq_rules.hpp"
#include "window_lanes.hpp"

namespace palace {
namespace {

constexpr int kQcThreads = 256, kQcWaves = kQcThreads / kWave;
constexpr int kQcGridCap = kCUs * 5 * 4;                 // the plan's workgroups: four times what is resident (32 KiB of LDS each)

static_assert(sizeof(palace_readqc_params) == 48, "params layout");
static_assert(kQcWaves * 2 * PALACE_FASTQ_MAX_SEQ == 32768, "a workgroup's LDS");

// what one lane wrote to LDS is read by another lane of the same wavefront: nothing but the order of the wave's own instructions is needed
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the records -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kQcThreads) void fastq_records_kernel(const uint8_t *t, const int64_t *start, int64_t n_records, int32_t *seq_len,
                                                                   unsigned long long *err)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kQcWaves + wave;
    if (r >= n_records) return;
    int64_t b[4], e[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { b[k] = start[4 * r + k]; e[k] = start[4 * r + k + 1] - 1; }
    const int64_t l_seq = e[1] - b[1], l_qual = e[3] - b[3];
    const bool too_long = l_seq > PALACE_FASTQ_MAX_SEQ;
    bool bad_base = false, bad_qual = false;
    if (!too_long) {
        for (int64_t p = b[1]; p < e[1]; p += kWave) {
            const int64_t q = p + lane;
            bad_base |= __ballot(q < e[1] && !fastq_base_ok(t[q])) != 0;
        }
        if (l_qual == l_seq)
            for (int64_t p = b[3]; p < e[3]; p += kWave) {
                const int64_t q = p + lane;
                bad_qual |= __ballot(q < e[3] && !fastq_qual_ok(t[q])) != 0;
            }
    }
    const FastqFault f = fastq_first_fault(e[0] == b[0] || t[b[0]] != '@', too_long, bad_base, e[2] == b[2] || t[b[2]] != '+', l_qual != l_seq, bad_qual);
    if (lane != 0) return;
    seq_len[r] = l_seq > INT32_MAX ? INT32_MAX : static_cast<int32_t>(l_seq);
    if (f.code) atomicMin(err, static_cast<unsigned long long>(4 * r + f.line + 1) << 3 | static_cast<unsigned long long>(f.code));
}

// ---- the pairs -------------------------------------------------------------------------------------------------------------------

// the first accepted candidate of the pair in the wave's LDS (-1: none); the same value in every lane
__device__ __forceinline__ int32_t first_accepted(const uint8_t *A, const uint8_t *B, int32_t l1, int32_t l2, const palace_readqc_params &p, int lane)
{
    const int32_t n_cand = fastq_forward_candidates(l1, p) + fastq_reverse_candidates(l2, p);
    for (int32_t c0 = 0; c0 < n_cand; c0 += kWave) {                        // (uniform: n_cand and c0 are the wave's)
        const int32_t c = c0 + lane;
        const bool mine = c < n_cand;
        FastqCand x{0, 0, 0};
        if (mine) x = fastq_candidate(c, l1, l2, p);
        const int32_t pct = x.n * p.diff_pct / 100, limit = p.diff_limit < pct ? p.diff_limit : pct, m = x.n < p.diff_window ? x.n : p.diff_window;
        int32_t diff = 0;
        for (int32_t i = 0; i < p.diff_window; i++) {                        // fastq_accept, the lanes in step
            const bool open = mine && i < m && diff <= limit;
            if (!__ballot(open)) break;
            if (open) diff += A[x.a0 + i] != B[x.b0 + i] ? 1 : 0;
        }
        const unsigned long long hit = __ballot(mine && diff <= limit);
        if (hit) return c0 + __ffsll(static_cast<long long>(hit)) - 1;
    }
    return -1;
}

// low QUAL bytes and N bases among the first `keep` of a read whose QUAL begins at t + q0 and whose bases are s[0], s[step], ...
__device__ __forceinline__ void prefix_counts(const uint8_t *t, int64_t q0, const uint8_t *s, int step, int32_t keep, uint32_t low_below, int lane, int32_t *low,
                                              int32_t *n_n)
{
    int32_t a = 0, b = 0;
    for (int32_t p = 0; p < keep; p += kWave) {
        const int32_t q = p + lane;
        a += __popcll(__ballot(q < keep && t[q0 + q] < low_below));
        b += __popcll(__ballot(q < keep && s[q * step] == 'N'));
    }
    *low = a; *n_n = b;
}

struct PairSums { unsigned long long v[9]; };

__global__ __launch_bounds__(kQcThreads) void readqc_plan_kernel(const uint8_t *t1, const int64_t *start1, const uint8_t *t2, const int64_t *start2, int64_t n_pairs,
                                                                 palace_readqc_params prm, int32_t *len1, int32_t *len2, int64_t *off1, int64_t *off2,
                                                                 unsigned long long *sums)
{
    __shared__ uint8_t s_ab[kQcWaves][2][PALACE_FASTQ_MAX_SEQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t *A = s_ab[wave][0], *B = s_ab[wave][1];
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kQcWaves;
    const uint32_t low_below = 33u + static_cast<uint32_t>(prm.qualified_quality);
    PairSums acc{};
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kQcWaves + wave; i < n_pairs; i += stride) {
        const int64_t a0 = start1[4 * i], a1 = start1[4 * i + 1], a2 = start1[4 * i + 2], a3 = start1[4 * i + 3], a4 = start1[4 * i + 4];
        const int64_t b0 = start2[4 * i], b1 = start2[4 * i + 1], b2 = start2[4 * i + 2], b3 = start2[4 * i + 3], b4 = start2[4 * i + 4];
        const int64_t w1 = a2 - 1 - a1, w2 = b2 - 1 - b1;
        if (w1 > PALACE_FASTQ_MAX_SEQ || w2 > PALACE_FASTQ_MAX_SEQ || w1 < 0 || w2 < 0 || a4 - 1 - a3 != w1 || b4 - 1 - b3 != w2) {
            // (not a text palace_fastq_records passed: nothing is staged, no QUAL byte is read)
            if (lane == 0) { len1[i] = len2[i] = -1; off1[i] = off2[i] = 0; }
            continue;
        }
        const int32_t l1 = static_cast<int32_t>(w1), l2 = static_cast<int32_t>(w2);
        wave_lds_sync();                                                     // (the pair before this one is done with A and B)
        for (int32_t j = lane; j < l1; j += kWave) A[j] = t1[a1 + j];
        for (int32_t j = lane; j < l2; j += kWave) B[j] = static_cast<uint8_t>(fastq_complement(t2[b1 + l2 - 1 - j]));
        wave_lds_sync();
        const int32_t c = prm.no_trim ? -1 : first_accepted(A, B, l1, l2, prm, lane);
        const int32_t cut = fastq_trim_to(c, l1, l2, prm);
        const int32_t k1 = cut >= 0 && cut < l1 ? cut : l1, k2 = cut >= 0 && cut < l2 ? cut : l2;
        int32_t low1, nn1, low2, nn2;
        prefix_counts(t1, a3, A, 1, k1, low_below, lane, &low1, &nn1);
        prefix_counts(t2, b3, B + (l2 > 0 ? l2 - 1 : 0), -1, k2, low_below, lane, &low2, &nn2);           // read 2's base q is B[l2 - 1 - q]; N stays N
        const int32_t reason = fastq_pair_reason(fastq_filter(k1, low1, nn1, prm), fastq_filter(k2, low2, nn2, prm));
        acc.v[PALACE_READQC_READS_BEFORE] += 2;
        acc.v[PALACE_READQC_BASES_BEFORE] += static_cast<unsigned long long>(l1 + l2);
        acc.v[PALACE_READQC_TRIMMED_READS] += (k1 < l1 ? 1 : 0) + (k2 < l2 ? 1 : 0);
        acc.v[PALACE_READQC_TRIMMED_BASES] += static_cast<unsigned long long>((l1 - k1) + (l2 - k2));
        acc.v[PALACE_READQC_LOW_QUALITY] += reason == kFastqLowQuality ? 2 : 0;
        acc.v[PALACE_READQC_TOO_MANY_N] += reason == kFastqTooManyN ? 2 : 0;
        acc.v[PALACE_READQC_TOO_SHORT] += reason == kFastqTooShort ? 2 : 0;
        acc.v[PALACE_READQC_READS_AFTER] += reason ? 0 : 2;
        acc.v[PALACE_READQC_BASES_AFTER] += reason ? 0 : static_cast<unsigned long long>(k1 + k2);
        if (lane == 0) {
            len1[i] = reason ? -1 : k1;
            len2[i] = reason ? -1 : k2;
            off1[i] = reason ? 0 : fastq_record_bytes(a1 - 1 - a0, a3 - 1 - a2, k1);
            off2[i] = reason ? 0 : fastq_record_bytes(b1 - 1 - b0, b3 - 1 - b2, k2);
        }
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 9; k++)
            if (acc.v[k]) atomicAdd(&sums[k], acc.v[k]);
}

// first launch of the two scans over the pairs: the sizes the plan left in off become the bytes in front, inside blocks of kScanThreads
__global__ __launch_bounds__(kScanThreads) void readqc_scan_kernel(int64_t n, int64_t *off1, int64_t *off2, long long *sum1, long long *sum2)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    long long t1, t2;
    const long long e1 = block_exclusive<long long, kScanThreads>(i < n ? off1[i] : 0, s_scan, &t1);
    const long long e2 = block_exclusive<long long, kScanThreads>(i < n ? off2[i] : 0, s_scan, &t2);
    if (i < n) { off1[i] = e1; off2[i] = e2; }
    if (threadIdx.x == 0) { sum1[blockIdx.x] = t1; sum2[blockIdx.x] = t2; }
}

// ---- the writer ------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kTileThreads) void readqc_write_kernel(const uint8_t *text, const int64_t *start, const int32_t *len, const int64_t *off, int64_t n_pairs,
                                                                    int64_t lo, int64_t hi, uint8_t *out)
{
    __shared__ long long s_rec[2];
    LaneOut l;
    int64_t p = window_lane(off, n_pairs, lo, hi, s_rec, &l);                // (behind dropped pairs it is a kept one)
    if (p < 0) return;
    while (!l.full()) {
        const int64_t n = len[p];
        const int64_t src[4] = {start[4 * p], start[4 * p + 1], start[4 * p + 2], start[4 * p + 3]};
        const int64_t ln[4] = {src[1] - 1 - src[0], n, src[3] - 1 - src[2], n};
        int64_t x = l.o0 + l.k - off[p];                                     // the byte's place in the record
#pragma unroll
        for (int s = 0; s < 4; s++) {
            if (l.full()) break;
            if (x > ln[s]) { x -= ln[s] + 1; continue; }
            if (l.k == 0 && l.cnt == kLaneBytes && x + kLaneBytes <= ln[s]) {    // the lane's 16 bytes are 16 neighbours of one line: one load, one store
                uint4 v;
                __builtin_memcpy(&v, text + src[s] + x, sizeof v);
                *reinterpret_cast<uint4 *>(out + l.j0) = v;
                return;
            }
            for (; x < ln[s] && !l.full(); x++) l.put(text[src[s] + x]);
            if (!l.full()) l.put('\n');
            x = 0;
        }
        if (l.full()) break;
        do p++; while (p < n_pairs && off[p + 1] == off[p]);                 // the next kept pair: bytes are left, so there is one
        if (p >= n_pairs) break;                                             // (hi beyond the text: the caller's fault, nothing is read for it)
    }
    l.store(out);
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_fastq_records(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, int32_t *d_seq_len, int64_t *out)
{
    PALACE_REQUIRE(ctx && n_lines >= 0 && out, "bad argument");
    const int64_t n_records = n_lines / 4;
    PALACE_REQUIRE(n_records < (1ll << 31), "more than 2^31 - 1 records");
    PALACE_REQUIRE(n_records == 0 || (d_text && d_line_start && d_seq_len), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long *err = reinterpret_cast<unsigned long long *>(ctx->d_small), e = ~0ull;
    if (n_records) {
        PALACE_HIP_TRY(hipMemcpyAsync(err, &e, sizeof e, hipMemcpyHostToDevice, ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                   // (e is this call's own)
        hipLaunchKernelGGL(fastq_records_kernel, dim3(static_cast<unsigned>((n_records + kQcWaves - 1) / kQcWaves)), dim3(kQcThreads), 0, ctx->stream, d_text,
                           d_line_start, n_records, d_seq_len, err);
        PALACE_HIP_TRY(hipGetLastError());
        PALACE_HIP_TRY(hipMemcpyAsync(&e, err, sizeof e, hipMemcpyDeviceToHost, ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    if (e == ~0ull && (n_lines & 3)) e = static_cast<unsigned long long>(4 * n_records + 1) << 3 | PALACE_FASTQ_ELINES;
    out[0] = n_records;
    out[1] = e == ~0ull ? 0 : static_cast<int64_t>(e >> 3);
    out[2] = e == ~0ull ? 0 : static_cast<int64_t>(e & 7);
    return PALACE_OK;
}

extern "C" int palace_readqc_plan(palace_ctx *ctx, const uint8_t *d_text1, const int64_t *d_line_start1, const uint8_t *d_text2, const int64_t *d_line_start2,
                                  int64_t n_pairs, const palace_readqc_params *prm, int32_t *d_len1, int32_t *d_len2, int64_t *d_off1, int64_t *d_off2, int64_t *out)
{
    PALACE_REQUIRE(ctx && n_pairs >= 0 && n_pairs < (1ll << 31) && prm && d_off1 && d_off2 && out, "bad argument");
    PALACE_REQUIRE(n_pairs == 0 || (d_text1 && d_text2 && d_line_start1 && d_line_start2 && d_len1 && d_len2), "null device pointer");
    PALACE_REQUIRE(prm->overlap_require >= 0 && prm->diff_limit >= 0 && prm->diff_pct >= 0 && prm->diff_pct <= 100 && prm->diff_window >= 0 &&
                       prm->diff_window <= PALACE_FASTQ_MAX_SEQ && prm->qualified_quality >= 0 && prm->qualified_quality <= 93 && prm->unqualified_percent >= 0 &&
                       prm->unqualified_percent <= 100 && prm->n_limit >= 0 && prm->min_length >= 0,
                   "a parameter out of range");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nb = (n_pairs + kScanThreads - 1) / kScanThreads;
    const int rc = ensure_workspace(ctx, 2 * static_cast<size_t>(nb + 1) * sizeof(long long));
    if (rc) return rc;
    long long *sum1 = static_cast<long long *>(ctx->ws.ptr), *sum2 = sum1 + nb + 1, bytes[2] = {0, 0};
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ctx->d_small), got[9] = {};
    PALACE_HIP_TRY(hipMemsetAsync(sums, 0, sizeof got, ctx->stream));
    if (nb == 0) {
        PALACE_HIP_TRY(hipMemsetAsync(d_off1, 0, sizeof(int64_t), ctx->stream));
        PALACE_HIP_TRY(hipMemsetAsync(d_off2, 0, sizeof(int64_t), ctx->stream));
    } else {
        const int64_t want = (n_pairs + kQcWaves - 1) / kQcWaves;
        hipLaunchKernelGGL(readqc_plan_kernel, dim3(static_cast<unsigned>(want < kQcGridCap ? want : kQcGridCap)), dim3(kQcThreads), 0, ctx->stream, d_text1,
                           d_line_start1, d_text2, d_line_start2, n_pairs, *prm, d_len1, d_len2, d_off1, d_off2, sums);
        hipLaunchKernelGGL(readqc_scan_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n_pairs, d_off1, d_off2, sum1, sum2);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sum1, nb);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sum2, nb);
        hipLaunchKernelGGL(add_block_base_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n_pairs, d_off1, sum1, nb);
        hipLaunchKernelGGL(add_block_base_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n_pairs, d_off2, sum2, nb);
        PALACE_HIP_TRY(hipGetLastError());
        PALACE_HIP_TRY(hipMemcpyAsync(&bytes[0], sum1 + nb, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        PALACE_HIP_TRY(hipMemcpyAsync(&bytes[1], sum2 + nb, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    }
    PALACE_HIP_TRY(hipMemcpyAsync(got, sums, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 9; k++) out[k] = static_cast<int64_t>(got[k]);
    out[PALACE_READQC_BYTES_1] = bytes[0];
    out[PALACE_READQC_BYTES_2] = bytes[1];
    return PALACE_OK;
}

extern "C" int palace_readqc_write(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, const int32_t *d_len, const int64_t *d_off, int64_t n_pairs,
                                   int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_pairs >= 0 && lo >= 0 && lo <= hi, "bad argument");
    if (lo == hi) return PALACE_OK;
    PALACE_REQUIRE(n_pairs > 0 && d_text && d_line_start && d_len && d_off && d_out, "null device pointer (or bytes asked of an empty text)");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (hi - lo + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE(nt < (1ll << 31), "window too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(readqc_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, d_line_start, d_len, d_off, n_pairs, lo, hi,
                       d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
