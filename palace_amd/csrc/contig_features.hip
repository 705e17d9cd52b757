// The input of the phage scorer (phage_scoring.py's encode.matrix_encoding(seq, 3); the rules: DESIGN.md 8): per record of an
// indexed FASTA three 64 x 64 count matrices of pairs of 3-mers that lie 3, 4 and 5 kept bases apart, scaled by 100 / length and
// written in the layout the model's first linear layer reads, and the row sums of the first matrix.
//
// A record's sequence S is addressed through its palace_fasta_rec (base p -> text offset), so the work is cut in CHUNKS of
// PALACE_CONTIG_CHUNK_BASES positions of S, whatever the line width.  A chunk is one workgroup in every chunk-sized launch:
//   1  chunks per record, scanned (3 launches): chunk_cum[0 .. R]
//   2  classify: kept bases (A C G T, either case) per chunk, and the smallest text offset of a digit
//   3  kept bases scanned over all chunks of the window (3 launches): kept_cum[0 .. NC] -- a chunk's place in the compact codes
//   4  scatter: the 2-bit codes of the kept bases, one per byte, records back to back
//   5  rows of records with more than one chunk are zeroed (as u32, in d_feat itself), records without a base of S get NaN
//   6  count: a chunk counts the pairs that START in it (it reads up to 7 codes beyond its own) into 12 288 u32 cells in LDS,
//      already in the model's layout; the only chunk of a record writes the row as float32, 16 bytes a lane; one of several adds
//      its non-zero cells into the record's zeroed row with global integer atomics
//   7  rows of records with more than one chunk become float32 in place
// Eleven launches whatever the text holds; every count is an integer until the last conversion, so the bytes do not depend on
// the order in which the atomics land.
#include <algorithm>

#include "scan64.hpp"

namespace palace {
namespace {

constexpr int kChunk = PALACE_CONTIG_CHUNK_BASES;
constexpr int kThreads = 256;
constexpr int kCells = PALACE_CONTIG_FEATURES;
static_assert(kChunk == kThreads * kLaneBytes, "a lane classifies 16 positions of S");
static_assert(kCells % (4 * kThreads) == 0, "rows are written 16 bytes a lane");

__host__ __device__ inline int64_t align16(int64_t v) { return (v + 15) & ~static_cast<int64_t>(15); }

struct Scratch {
    int64_t *chunk_cum;      // [R + 1]
    int64_t *kept_cum;       // [NC + 1]
    long long *sums;         // block sums of either scan
    uint8_t *codes;          // [n_text]
    int64_t nc;              // chunks at most: n_text / kChunk + R
};

inline int64_t chunks_cap(int64_t n_text, int64_t n_records) { return n_text / kChunk + n_records; }

inline size_t scratch_layout(int64_t n_text, int64_t n_records, uint8_t *base, Scratch *s)
{
    const int64_t nc = chunks_cap(n_text, n_records);
    const int64_t nb = (std::max(nc, n_records) + kScanThreads - 1) / kScanThreads;
    int64_t at = 0;
    const int64_t o_chunk = at; at = align16(at + (n_records + 1) * 8);
    const int64_t o_kept = at;  at = align16(at + (nc + 1) * 8);
    const int64_t o_sums = at;  at = align16(at + (nb + 1) * 8);
    const int64_t o_codes = at; at = align16(at + n_text);
    if (s) {
        s->chunk_cum = reinterpret_cast<int64_t *>(base + o_chunk);
        s->kept_cum = reinterpret_cast<int64_t *>(base + o_kept);
        s->sums = reinterpret_cast<long long *>(base + o_sums);
        s->codes = base + o_codes;
        s->nc = nc;
    }
    return static_cast<size_t>(at);
}

// ---- the scans ---------------------------------------------------------------------------------------------------------------

struct ChunksOf {
    const palace_fasta_rec *recs;      // the window's first record
    __device__ __forceinline__ long long operator()(int64_t j) const
    {
        const palace_fasta_rec rec = recs[j];
        if (rec.length <= 0 || rec.line_bases <= 0 || rec.line_width < rec.line_bases) return 0;      // (no record of a sound index with bases)
        return (rec.length + kChunk - 1) / kChunk;
    }
};
struct ValueAt {
    const int64_t *v;                  // the array that is scanned in place
    __device__ __forceinline__ long long operator()(int64_t c) const { return v[c]; }
};

// ---- a lane's 16 positions of S ----------------------------------------------------------------------------------------------

// 0..3 for A C G T in either case, 4 for a digit, 5 for every other byte
__device__ __forceinline__ int base_class(uint32_t b)
{
    const uint32_t u = b & 0xdfu;                  // upper case of a letter
    if (u == 'A') return 0;
    if (u == 'C') return 1;
    if (u == 'G') return 2;
    if (u == 'T') return 3;
    return b - '0' < 10u ? 4 : 5;
}

// The chunk's record and its first position of S; false when the chunk does not exist
struct ChunkAt {
    int64_t j, p0, first_chunk, n_chunks;
};
__device__ __forceinline__ bool chunk_at(const int64_t *chunk_cum, int64_t n_rec, int64_t c, ChunkAt *out)
{
    if (c >= chunk_cum[n_rec]) return false;
    const int64_t j = last_le(chunk_cum, 0, n_rec - 1, c);
    out->j = j;
    out->first_chunk = chunk_cum[j];
    out->n_chunks = chunk_cum[j + 1] - chunk_cum[j];
    out->p0 = (c - chunk_cum[j]) * kChunk;
    return true;
}

// Classes of the lane's positions [p, min(p + 16, length)) of the record, four bits each in *cls; the number of positions.
// first_digit_at: the text offset of the lane's first digit, or -1.
__device__ __forceinline__ int lane_classes(const uint8_t *text, int64_t n, const palace_fasta_rec &rec, int64_t p, uint64_t *cls,
                                            int64_t *first_digit_at)
{
    *cls = 0;
    *first_digit_at = -1;
    if (p >= rec.length) return 0;
    const int cnt = static_cast<int>(rec.length - p < kLaneBytes ? rec.length - p : kLaneBytes);
    int64_t line = p / rec.line_bases, col = p - line * rec.line_bases;        // length > 0: the record has a first line with bases
    int64_t at = rec.seq_off + line * rec.line_width + col;
    for (int k = 0; k < cnt; k++) {
        const int cl = at >= 0 && at < n ? base_class(text[at]) : 5;                       // (a record of a sound index ends inside the text)
        *cls |= static_cast<uint64_t>(cl) << (4 * k);
        if (cl == 4 && *first_digit_at < 0) *first_digit_at = at;
        if (++col == rec.line_bases) { col = 0; at += rec.line_width - rec.line_bases + 1; } else at++;
    }
    return cnt;
}

__device__ __forceinline__ int kept_of(uint64_t cls, int cnt)
{
    int kept = 0;
    for (int k = 0; k < cnt; k++) kept += ((cls >> (4 * k)) & 15u) < 4u;
    return kept;
}

// ---- the chunk-sized launches -------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void contig_classify_kernel(const uint8_t *text, int64_t n, const palace_fasta_rec *recs, int64_t n_rec,
                                                                  const int64_t *chunk_cum, int64_t *kept, unsigned long long *bad)
{
    __shared__ int s_kept;
    const int64_t c = blockIdx.x;
    ChunkAt ch;
    if (!chunk_at(chunk_cum, n_rec, c, &ch)) {
        if (threadIdx.x == 0) kept[c] = 0;
        return;
    }
    if (threadIdx.x == 0) s_kept = 0;
    __syncthreads();
    const palace_fasta_rec rec = recs[ch.j];
    uint64_t cls;
    int64_t digit_at;
    const int cnt = lane_classes(text, n, rec, ch.p0 + static_cast<int64_t>(threadIdx.x) * kLaneBytes, &cls, &digit_at);
    const int k = kept_of(cls, cnt);
    if (k) atomicAdd(&s_kept, k);
    if (digit_at >= 0) atomicMin(bad, static_cast<unsigned long long>(digit_at));
    __syncthreads();
    if (threadIdx.x == 0) kept[c] = s_kept;
}

__global__ __launch_bounds__(kThreads) void contig_scatter_kernel(const uint8_t *text, int64_t n, const palace_fasta_rec *recs, int64_t n_rec,
                                                                 const int64_t *chunk_cum, const int64_t *kept_cum, uint8_t *codes)
{
    __shared__ int s_scan[kThreads / 64 + 1];
    const int64_t c = blockIdx.x;
    ChunkAt ch;
    if (!chunk_at(chunk_cum, n_rec, c, &ch)) return;
    const palace_fasta_rec rec = recs[ch.j];
    uint64_t cls;
    int64_t digit_at;
    const int cnt = lane_classes(text, n, rec, ch.p0 + static_cast<int64_t>(threadIdx.x) * kLaneBytes, &cls, &digit_at);
    int total;
    const int ex = block_exclusive<int, kThreads>(kept_of(cls, cnt), s_scan, &total);
    int64_t out = kept_cum[c] + ex;
    for (int k = 0; k < cnt; k++) {
        const uint32_t cl = (cls >> (4 * k)) & 15u;
        if (cl < 4u && out < n) codes[out++] = static_cast<uint8_t>(cl);            // (out < n: the records of a sound index do not overlap)
    }
}

// one workgroup per record: the row of a record with several chunks is zeroed for the counts, a record without a position of S
// gets what 0 / 0 gives; d_info
__global__ __launch_bounds__(kThreads) void contig_rows_begin_kernel(const palace_fasta_rec *recs, const int64_t *chunk_cum, const int64_t *kept_cum,
                                                                    float *feat, float *fsum, palace_contig_info *info)
{
    const int64_t j = blockIdx.x;
    const int64_t c0 = chunk_cum[j], c1 = chunk_cum[j + 1];
    if (info && threadIdx.x == 0) {
        info[j].length = recs[j].length;
        info[j].bases = kept_cum[c1] - kept_cum[c0];
    }
    if (c1 - c0 == 1) return;
    uint4 fill = {0u, 0u, 0u, 0u};
    if (c1 == c0) {
        const double zero = 0.0;
        const float v = static_cast<float>(zero / static_cast<double>(recs[j].length) * 100.0);      // length 0 (or below): NaN
        fill.x = fill.y = fill.z = fill.w = __float_as_uint(v);
        if (threadIdx.x < PALACE_CONTIG_FSUMS) fsum[j * PALACE_CONTIG_FSUMS + threadIdx.x] = v;
    }
    uint4 *row = reinterpret_cast<uint4 *>(feat + j * kCells);
    for (int q = threadIdx.x; q < kCells / 4; q += kThreads) row[q] = fill;
}

__device__ __forceinline__ float scaled(uint32_t count, double length) { return static_cast<float>(static_cast<double>(count) / length * 100.0); }

__global__ __launch_bounds__(kThreads) void contig_count_kernel(const palace_fasta_rec *recs, int64_t n_rec, const int64_t *chunk_cum,
                                                               const int64_t *kept_cum, const uint8_t *codes, float *feat, float *fsum)
{
    __shared__ uint32_t s_cell[kCells];              // cell (d, a, b) at (a * 64 + b) * 3 + d
    const int64_t c = blockIdx.x;
    ChunkAt ch;
    if (!chunk_at(chunk_cum, n_rec, c, &ch)) return;
    const int64_t k0 = kept_cum[c], k1 = kept_cum[c + 1];
    if (ch.n_chunks > 1 && k0 == k1) return;
    const int64_t rec_k1 = kept_cum[ch.first_chunk + ch.n_chunks];
    for (int q = threadIdx.x; q < kCells; q += kThreads) s_cell[q] = 0;
    __syncthreads();
    // pair (i, i + 3 + d) of a record whose codes end before rec_k1 exists for i + 5 + d < rec_k1: its last base is code i + 5 + d
    for (int64_t i = k0 + threadIdx.x; i < k1 && i + 5 < rec_k1; i += kThreads) {
        const uint8_t *v = codes + i;
        const int avail = static_cast<int>(rec_k1 - i < 8 ? rec_k1 - i : 8);        // 6, 7 or 8
        const uint32_t a = 16u * v[0] + 4u * v[1] + v[2];
        uint32_t w = 16u * v[3] + 4u * v[4] + v[5];
        atomicAdd(&s_cell[(a * 64 + w) * 3 + 0], 1u);
        if (avail > 6) {
            w = (w * 4 + v[6]) & 63u;
            atomicAdd(&s_cell[(a * 64 + w) * 3 + 1], 1u);
            if (avail > 7) {
                w = (w * 4 + v[7]) & 63u;
                atomicAdd(&s_cell[(a * 64 + w) * 3 + 2], 1u);
            }
        }
    }
    __syncthreads();
    if (ch.n_chunks == 1) {
        const double length = static_cast<double>(recs[ch.j].length);
        float4 *row = reinterpret_cast<float4 *>(feat + ch.j * kCells);
        for (int q = threadIdx.x; q < kCells / 4; q += kThreads) {
            float4 o;
            o.x = scaled(s_cell[4 * q], length); o.y = scaled(s_cell[4 * q + 1], length);
            o.z = scaled(s_cell[4 * q + 2], length); o.w = scaled(s_cell[4 * q + 3], length);
            row[q] = o;
        }
        if (threadIdx.x < PALACE_CONTIG_FSUMS) {
            uint32_t sum = 0;
            for (int b = 0; b < 64; b++) sum += s_cell[(threadIdx.x * 64 + b) * 3];
            fsum[ch.j * PALACE_CONTIG_FSUMS + threadIdx.x] = scaled(sum, length);
        }
    } else {
        unsigned int *row = reinterpret_cast<unsigned int *>(feat + ch.j * kCells);
        for (int q = threadIdx.x; q < kCells; q += kThreads)
            if (s_cell[q]) atomicAdd(&row[q], s_cell[q]);
    }
}

// one workgroup per record: the u32 counts of a record with several chunks become its features, in place
__global__ __launch_bounds__(kThreads) void contig_rows_end_kernel(const palace_fasta_rec *recs, const int64_t *chunk_cum, float *feat, float *fsum)
{
    const int64_t j = blockIdx.x;
    if (chunk_cum[j + 1] - chunk_cum[j] < 2) return;
    const double length = static_cast<double>(recs[j].length);
    uint4 *row = reinterpret_cast<uint4 *>(feat + j * kCells);
    if (threadIdx.x < PALACE_CONTIG_FSUMS) {
        const uint32_t *cell = reinterpret_cast<const uint32_t *>(row);
        uint32_t sum = 0;
        for (int b = 0; b < 64; b++) sum += cell[(threadIdx.x * 64 + b) * 3];
        fsum[j * PALACE_CONTIG_FSUMS + threadIdx.x] = scaled(sum, length);
    }
    __syncthreads();                                 // the sums are read before any cell of the row changes its meaning
    for (int q = threadIdx.x; q < kCells / 4; q += kThreads) {
        uint4 v = row[q];
        v.x = __float_as_uint(scaled(v.x, length)); v.y = __float_as_uint(scaled(v.y, length));
        v.z = __float_as_uint(scaled(v.z, length)); v.w = __float_as_uint(scaled(v.w, length));
        row[q] = v;
    }
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_contig_features_scratch_bytes(int64_t n_text, int64_t n_records)
{
    if (n_text < 0 || n_records < 0) return 0;
    return scratch_layout(n_text, n_records, nullptr, nullptr);
}

extern "C" int palace_contig_features(palace_ctx *ctx, const uint8_t *d_text, int64_t n, const palace_fasta_rec *d_recs, int64_t r0, int64_t r1,
                                      float *d_feat, float *d_fsum, palace_contig_info *d_info, int64_t *d_bad, void *d_scratch, size_t scratch_bytes)
{
    PALACE_REQUIRE(ctx && d_bad && n >= 0 && r0 >= 0 && r0 <= r1, "bad arguments");
    PALACE_HIP_TRY(hipMemsetAsync(d_bad, 0xff, sizeof(int64_t), ctx->stream));          // -1, and the largest offset for atomicMin
    const int64_t n_rec = r1 - r0;
    if (n_rec == 0) return PALACE_OK;
    PALACE_REQUIRE(d_text && d_recs && d_feat && d_fsum && d_scratch, "null buffer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_feat) & 15) == 0 && (reinterpret_cast<uintptr_t>(d_scratch) & 15) == 0, "d_feat and d_scratch: 16-byte aligned");
    Scratch s;
    PALACE_REQUIRE(scratch_bytes >= scratch_layout(n, n_rec, static_cast<uint8_t *>(d_scratch), &s), "scratch too small");
    PALACE_REQUIRE(s.nc < (1ll << 31) && n_rec < (1ll << 31), "too many chunks or records for one call");
    const palace_fasta_rec *recs = d_recs + r0;
    const dim3 chunks(static_cast<unsigned>(s.nc)), records(static_cast<unsigned>(n_rec)), threads(kThreads);

    scan_sizes_into(ctx, ChunksOf{recs}, n_rec, s.chunk_cum, s.sums);
    hipLaunchKernelGGL(contig_classify_kernel, chunks, threads, 0, ctx->stream, d_text, n, recs, n_rec, s.chunk_cum, s.kept_cum,
                       reinterpret_cast<unsigned long long *>(d_bad));
    scan_sizes_into(ctx, ValueAt{s.kept_cum}, s.nc, s.kept_cum, s.sums);
    hipLaunchKernelGGL(contig_scatter_kernel, chunks, threads, 0, ctx->stream, d_text, n, recs, n_rec, s.chunk_cum, s.kept_cum, s.codes);
    hipLaunchKernelGGL(contig_rows_begin_kernel, records, threads, 0, ctx->stream, recs, s.chunk_cum, s.kept_cum, d_feat, d_fsum, d_info);
    hipLaunchKernelGGL(contig_count_kernel, chunks, threads, 0, ctx->stream, recs, n_rec, s.chunk_cum, s.kept_cum, s.codes, d_feat, d_fsum);
    hipLaunchKernelGGL(contig_rows_end_kernel, records, threads, 0, ctx->stream, recs, s.chunk_cum, d_feat, d_fsum);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
