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
//
// The report (readqc --full-report).  The plan kernel gets no LDS for it: its 32 KiB are exactly five workgroups of a CU.  It only
// stores the candidate it found (palace_readqc_plan_ex; the store is a template parameter, so palace_readqc_plan's kernel is the one
// it was), and what is counted is counted by two kernels of their own.
//   The cycles (palace_readqc_cycle_stats).  A workgroup of 256 threads owns a tile of 256 cycles (grid y) and a share of the reads
//   (grid x, four neighbouring reads a step); thread t owns cycle 256 y + t, so a wavefront reads 64 neighbouring bytes of SEQ and 64 of
//   QUAL of a read, and every byte is read once.  A thread's counters (5 counts, 5 QUAL sums, Q20, Q30) are 32-bit registers across all
//   the reads its workgroup walks.  A second set counts the cycles BEHIND a read's kept length and "after" is the difference: an
//   untrimmed read of a kept pair -- most reads -- is counted once, and a wavefront skips, as one, a read that ends before its cycles.
//   A workgroup walks at most 2^31 / 2048 + 4 reads when the grid is at its cap and a QUAL value is at most 93, so no counter passes
//   2^27.  The slot is compared, not indexed, so the counters stay registers (48 VGPRs, no scratch, 8 waves a SIMD).
//   At the end a workgroup turns its counters through 5 KiB of LDS into the table's own order ([cycle][slot], 5 dwords a thread: stride
//   5 is free of bank conflicts) and adds them with 64-bit atomics, 512 neighbouring bytes a wave instruction, zeros left out: 2048
//   workgroups x 256 cycles x 20 words at the most, whatever the text's size.  The sums are integers: the order of the adds is
//   nothing to the result.  Bytes: SEQ + QUAL once, 32 B of line starts a read and tile (uniform loads), 4 B of kept length.  The
//   floor is HBM (1.12 GB a text of the 1M-contig sample: 0.14 ms); measured 1.78 ms with kept lengths (8 % of it), 1.58 ms without (9 %):
//   the bound is instruction issue -- some 45 vector instructions a wavefront and read, half of the time -- and the two dependent
//   loads of a step (the line starts, then the bytes), not memory (profiles/readqc.md).
//   The insert sizes (palace_readqc_insert_sizes).  A thread takes a pair: two line starts of either text and the candidate in, one
//   LDS atomic on the workgroup's 513 x 4 B histogram; the histogram leaves the workgroup once, zeros left out.
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

// kCand: the pair's candidate goes to cand[] (the report's insert sizes); without it this is the kernel as it was
template <bool kCand>
__global__ __launch_bounds__(kQcThreads) void readqc_plan_kernel(const uint8_t *t1, const int64_t *start1, const uint8_t *t2, const int64_t *start2, int64_t n_pairs,
                                                                 palace_readqc_params prm, int32_t *len1, int32_t *len2, int64_t *off1, int64_t *off2,
                                                                 unsigned long long *sums, int32_t *cand)
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
            if (kCand && lane == 0) cand[i] = -1;
            continue;
        }
        const int32_t l1 = static_cast<int32_t>(w1), l2 = static_cast<int32_t>(w2);
        wave_lds_sync();                                                     // (the pair before this one is done with A and B)
        for (int32_t j = lane; j < l1; j += kWave) A[j] = t1[a1 + j];
        for (int32_t j = lane; j < l2; j += kWave) B[j] = static_cast<uint8_t>(fastq_complement(t2[b1 + l2 - 1 - j]));
        wave_lds_sync();
        const int32_t c = prm.no_trim ? -1 : first_accepted(A, B, l1, l2, prm, lane);
        if (kCand && lane == 0) cand[i] = c;                                 // (dropped pairs too: the insert size is the input's)
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

// ---- the report ------------------------------------------------------------------------------------------------------------------

constexpr int kCycleTile = 256;                          // the cycles, and the threads, of a workgroup of the cycle statistics
constexpr int kCycleReads = 4;                           // neighbouring reads whose bytes a thread has in flight
constexpr int kCycleGridCap = kCUs * 8;                  // workgroups per cycle tile: the 32 waves of a CU (55 VGPRs)
static_assert(kCycleGridCap >= 64, "the 32-bit counters: (2^31 / cap + kCycleReads) reads x 93 stays below 2^32");
constexpr int kIsizeThreads = 256, kIsizeGridCap = kCUs * 4;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

struct CycleCounts { uint32_t cnt[kFastqSlots], qsum[kFastqSlots], q20, q30; };

__device__ __forceinline__ void cycle_count(CycleCounts &c, bool on, uint32_t base, uint32_t qual)
{
    const int32_t slot = fastq_base_slot(base);
    const uint32_t v = fastq_qual_value(qual);
#pragma unroll
    for (int k = 0; k < kFastqSlots; k++) {                                  // (compared, not indexed: the counters stay registers)
        const bool hit = on && slot == k;
        c.cnt[k] += hit ? 1u : 0u;
        c.qsum[k] += hit ? v : 0u;
    }
    c.q20 += on && fastq_is_q20(qual) ? 1u : 0u;
    c.q30 += on && fastq_is_q30(qual) ? 1u : 0u;
}

// the workgroup's counters of one table of one section -> sec[0 .. 5 * max_cycles), in the table's order through s_turn
__device__ __forceinline__ void cycle_flush(const uint32_t (&mine)[kFastqSlots], uint32_t *s_turn, unsigned long long *table, int32_t tile0, int32_t max_cycles)
{
    __syncthreads();                                                         // (the table before this one is read)
#pragma unroll
    for (int k = 0; k < kFastqSlots; k++) s_turn[threadIdx.x * kFastqSlots + k] = mine[k];
    __syncthreads();
    const int32_t cycles = max_cycles - tile0 < kCycleTile ? max_cycles - tile0 : kCycleTile;
    for (int32_t j = threadIdx.x; j < cycles * kFastqSlots; j += kCycleTile)
        if (s_turn[j]) atomicAdd(&table[static_cast<int64_t>(tile0) * kFastqSlots + j], static_cast<unsigned long long>(s_turn[j]));
}

template <bool kAfter>
__global__ __launch_bounds__(kCycleTile) void readqc_cycle_stats_kernel(const uint8_t *__restrict__ t, const int64_t *__restrict__ start, int64_t n_records,
                                                                        const int32_t *__restrict__ len, int32_t max_cycles, unsigned long long *out)
{
    __shared__ uint32_t s_turn[kCycleTile * kFastqSlots];
    const int32_t tile0 = static_cast<int32_t>(blockIdx.y) * kCycleTile, cycle = tile0 + static_cast<int32_t>(threadIdx.x);
    const int32_t wave0 = __builtin_amdgcn_readfirstlane(cycle);            // the wavefront's first cycle: what it skips, it skips as one
    const int64_t step = static_cast<int64_t>(gridDim.x) * kCycleReads;
    CycleCounts before{}, lost{};                                            // lost: the cycles behind a read's kept length; after = before - lost
    for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * kCycleReads; r0 < n_records; r0 += step) {        // (uniform: the workgroup's reads)
        uint32_t base[kCycleReads], qual[kCycleReads];
        bool in[kCycleReads], cut[kCycleReads];
#pragma unroll
        for (int u = 0; u < kCycleReads; u++) {
            const int64_t r = r0 + u;
            in[u] = cut[u] = false;
            base[u] = qual[u] = 0;
            if (r >= n_records || wave0 >= max_cycles) continue;
            const int64_t s1 = start[4 * r + 1], s2 = start[4 * r + 2], s3 = start[4 * r + 3], s4 = start[4 * r + 4];
            const int64_t l = s2 - 1 - s1;
            if (l <= wave0 || s4 - 1 - s3 != l) continue;                    // (a read that ends before the wave's cycles; or not a text palace_fastq_records passed)
            in[u] = cycle < l && cycle < max_cycles;
            if (in[u]) { base[u] = t[s1 + cycle]; qual[u] = t[s3 + cycle]; }
            if (kAfter) cut[u] = in[u] && cycle >= len[r];                   // (-1, a dropped pair: every cycle is behind it)
        }
#pragma unroll
        for (int u = 0; u < kCycleReads; u++) {
            if (__ballot(in[u])) cycle_count(before, in[u], base[u], qual[u]);
            if (kAfter && __ballot(cut[u])) cycle_count(lost, cut[u], base[u], qual[u]);        // (an untrimmed read of a kept pair is counted once)
        }
    }
    CycleCounts after = before;
    if (kAfter) {
#pragma unroll
        for (int k = 0; k < kFastqSlots; k++) { after.cnt[k] -= lost.cnt[k]; after.qsum[k] -= lost.qsum[k]; }
        after.q20 -= lost.q20;
        after.q30 -= lost.q30;
    }
    const int64_t tables = static_cast<int64_t>(kFastqSlots) * max_cycles, words = PALACE_READQC_SECTION_WORDS(max_cycles);
    for (int s = 0; s < (kAfter ? 2 : 1); s++) {
        const CycleCounts &c = s ? after : before;
        unsigned long long *sec = out + s * words;
        cycle_flush(c.cnt, s_turn, sec, tile0, max_cycles);
        cycle_flush(c.qsum, s_turn, sec + tables, tile0, max_cycles);
        const uint32_t n20 = wave_sum(c.q20), n30 = wave_sum(c.q30);
        if ((threadIdx.x & 63) == 0) {
            if (n20) atomicAdd(&sec[2 * tables], static_cast<unsigned long long>(n20));
            if (n30) atomicAdd(&sec[2 * tables + 1], static_cast<unsigned long long>(n30));
        }
    }
}

__global__ __launch_bounds__(kIsizeThreads) void readqc_insert_sizes_kernel(const int64_t *__restrict__ start1, const int64_t *__restrict__ start2,
                                                                            const int32_t *__restrict__ cand, int64_t n_pairs, palace_readqc_params prm,
                                                                            unsigned long long *hist)
{
    __shared__ uint32_t s_hist[PALACE_READQC_ISIZE_MAX + 1];                 // (a workgroup strides at most 2^31 / 256 pairs: 32 bits hold them)
    for (int j = threadIdx.x; j <= PALACE_READQC_ISIZE_MAX; j += kIsizeThreads) s_hist[j] = 0;
    __syncthreads();
    const int64_t stride = static_cast<int64_t>(gridDim.x) * kIsizeThreads;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kIsizeThreads + threadIdx.x; i < n_pairs; i += stride) {
        const int64_t w1 = start1[4 * i + 2] - 1 - start1[4 * i + 1], w2 = start2[4 * i + 2] - 1 - start2[4 * i + 1];
        int32_t size = PALACE_READQC_ISIZE_MAX;
        if (w1 >= 0 && w2 >= 0 && w1 <= PALACE_FASTQ_MAX_SEQ && w2 <= PALACE_FASTQ_MAX_SEQ) {
            const int32_t l1 = static_cast<int32_t>(w1), l2 = static_cast<int32_t>(w2), c = cand[i];
            if (c < fastq_forward_candidates(l1, prm) + fastq_reverse_candidates(l2, prm)) size = fastq_insert_size(c, l1, l2, prm);
        }
        if (size < 0 || size > PALACE_READQC_ISIZE_MAX) size = PALACE_READQC_ISIZE_MAX;          // (whatever cand[] held, the slot is one of the 513)
        atomicAdd(&s_hist[size], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j <= PALACE_READQC_ISIZE_MAX; j += kIsizeThreads)
        if (s_hist[j]) atomicAdd(&hist[j], static_cast<unsigned long long>(s_hist[j]));
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

static bool readqc_params_ok(const palace_readqc_params *prm)
{
    return prm->overlap_require >= 0 && prm->diff_limit >= 0 && prm->diff_pct >= 0 && prm->diff_pct <= 100 && prm->diff_window >= 0 &&
           prm->diff_window <= PALACE_FASTQ_MAX_SEQ && prm->qualified_quality >= 0 && prm->qualified_quality <= 93 && prm->unqualified_percent >= 0 &&
           prm->unqualified_percent <= 100 && prm->n_limit >= 0 && prm->min_length >= 0;
}

extern "C" int palace_readqc_plan_ex(palace_ctx *ctx, const uint8_t *d_text1, const int64_t *d_line_start1, const uint8_t *d_text2, const int64_t *d_line_start2,
                                     int64_t n_pairs, const palace_readqc_params *prm, int32_t *d_len1, int32_t *d_len2, int64_t *d_off1, int64_t *d_off2,
                                     int32_t *d_cand, int64_t *out)
{
    PALACE_REQUIRE(ctx && n_pairs >= 0 && n_pairs < (1ll << 31) && prm && d_off1 && d_off2 && out, "bad argument");
    PALACE_REQUIRE(n_pairs == 0 || (d_text1 && d_text2 && d_line_start1 && d_line_start2 && d_len1 && d_len2), "null device pointer");
    PALACE_REQUIRE(readqc_params_ok(prm), "a parameter out of range");
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
        hipLaunchKernelGGL(d_cand ? readqc_plan_kernel<true> : readqc_plan_kernel<false>, dim3(static_cast<unsigned>(want < kQcGridCap ? want : kQcGridCap)),
                           dim3(kQcThreads), 0, ctx->stream, d_text1, d_line_start1, d_text2, d_line_start2, n_pairs, *prm, d_len1, d_len2, d_off1, d_off2, sums, d_cand);
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

extern "C" int palace_readqc_plan(palace_ctx *ctx, const uint8_t *d_text1, const int64_t *d_line_start1, const uint8_t *d_text2, const int64_t *d_line_start2,
                                  int64_t n_pairs, const palace_readqc_params *prm, int32_t *d_len1, int32_t *d_len2, int64_t *d_off1, int64_t *d_off2, int64_t *out)
{
    return palace_readqc_plan_ex(ctx, d_text1, d_line_start1, d_text2, d_line_start2, n_pairs, prm, d_len1, d_len2, d_off1, d_off2, nullptr, out);
}

extern "C" int palace_readqc_insert_sizes(palace_ctx *ctx, const int64_t *d_line_start1, const int64_t *d_line_start2, const int32_t *d_cand, int64_t n_pairs,
                                          const palace_readqc_params *prm, uint64_t *d_hist)
{
    PALACE_REQUIRE(ctx && n_pairs >= 0 && n_pairs < (1ll << 31) && prm && d_hist, "bad argument");
    PALACE_REQUIRE(n_pairs == 0 || (d_line_start1 && d_line_start2 && d_cand), "null device pointer");
    PALACE_REQUIRE(readqc_params_ok(prm), "a parameter out of range");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    PALACE_HIP_TRY(hipMemsetAsync(d_hist, 0, (PALACE_READQC_ISIZE_MAX + 1) * sizeof(uint64_t), ctx->stream));
    if (n_pairs == 0) return PALACE_OK;
    const int64_t want = (n_pairs + kIsizeThreads - 1) / kIsizeThreads;
    hipLaunchKernelGGL(readqc_insert_sizes_kernel, dim3(static_cast<unsigned>(want < kIsizeGridCap ? want : kIsizeGridCap)), dim3(kIsizeThreads), 0, ctx->stream,
                       d_line_start1, d_line_start2, d_cand, n_pairs, *prm, reinterpret_cast<unsigned long long *>(d_hist));
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_readqc_cycle_stats(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_records, const int32_t *d_len,
                                         int32_t max_cycles, uint64_t *d_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && max_cycles >= 0 && max_cycles <= PALACE_FASTQ_MAX_SEQ && d_out, "bad argument");
    PALACE_REQUIRE(n_records == 0 || (d_text && d_line_start), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t words = static_cast<size_t>(PALACE_READQC_SECTION_WORDS(max_cycles)) * (d_len ? 2 : 1);
    PALACE_HIP_TRY(hipMemsetAsync(d_out, 0, words * sizeof(uint64_t), ctx->stream));
    if (n_records == 0 || max_cycles == 0) return PALACE_OK;
    const int64_t want = (n_records + kCycleReads - 1) / kCycleReads;
    const dim3 grid(static_cast<unsigned>(want < kCycleGridCap ? want : kCycleGridCap), static_cast<unsigned>((max_cycles + kCycleTile - 1) / kCycleTile));
    hipLaunchKernelGGL(d_len ? readqc_cycle_stats_kernel<true> : readqc_cycle_stats_kernel<false>, grid, dim3(kCycleTile), 0, ctx->stream, d_text, d_line_start,
                       n_records, d_len, max_cycles, reinterpret_cast<unsigned long long *>(d_out));
    PALACE_HIP_TRY(hipGetLastError());
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
