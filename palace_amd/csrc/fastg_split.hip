// FASTG -> node FASTA on the device (include/palace_hip.h: palace_fastg_derive .. palace_fai_rows_write): what the reference's
// split_fastg.py does line by line, and the `.fai` rows that `samtools faidx` writes behind it.  The rules: DESIGN.md 8.
//
// The text is indexed by palace_fasta_index (path_fasta.hip); what is new here:
//   derive: one lane per record walks the header token up to its first ':' ',' ' ' or line end and leaves the record's name (the
//           token without its last byte, cut at the first ':' or ',', without a closing ') and the primed bit; one lane per 16
//           bytes of text judges its own bytes -- a sequence line's first byte, a header line's bytes, the bases of primed
//           records -- knowing its record from one search per tile and one per lane.  A fault is kept as the smallest OFFSET
//           per code; the lines of those offsets are counted afterwards (only a text at fault pays for that), so the verdict
//           does not depend on tiling.
//   plan:   a 64-bit scan of the kept records' output sizes (a dropped record has none; scan64.hpp).
//   write:  any window [lo, hi) of the output, by the lanes, the gather and the upper-casing complement of window_lanes.hpp: the
//           items are the kept records, a primed record is read from its end.
//   rows:   length pass, scan, write of the five-column index rows, one lane per row.
#include "common.hpp"
#include "window_lanes.hpp"

#include <climits>

namespace palace {
namespace {

constexpr int kCodes = 16;                       // fault codes are below this
// ctx->d_small, in 64-bit words: the smallest offset per fault code, the line ends in front of each, and the plan's two words
constexpr int kOffAt = 0, kLinesAt = kCodes, kFirstEmptyAt = 2 * kCodes, kKeptAt = 2 * kCodes + 1;

static_assert(PALACE_FASTG_EBASE < kCodes && 2 * kCodes + 2 <= 64, "the faults fit the context's small scratch");

struct Offsets { long long at[kCodes]; };

__device__ __forceinline__ void fault_at(unsigned long long *small, int code, int64_t off)
{
    atomicMin(&small[kOffAt + code], static_cast<unsigned long long>(off));
}

__device__ __forceinline__ bool is_base(uint32_t c)
{
    const uint32_t u = c & 0xdfu;
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}

// ---- derive ---------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void fastg_names_kernel(const uint8_t *text, int64_t n, const palace_fasta_rec *recs, int64_t n_records,
                                                          palace_fasta_rec *name_recs, uint8_t *primed, unsigned long long *small)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= n_records) return;
    palace_fasta_rec rec = recs[r];
    const int64_t s = rec.name_off;
    int64_t j = s;
    while (j < n && text[j] != ':' && text[j] != ',' && text[j] != ' ' && text[j] != '\n') j++;
    int64_t v = j - s;                                                       // a ':' or ',' lies inside the token: the name ends in front of it
    if (j >= n || text[j] == ' ' || text[j] == '\n') {                       // the token's end: its last byte is not the name's
        if (j < n && text[j] == '\n' && j > s && text[j - 1] == '\r') v--;   // (a CR directly before the LF is not the line's)
        v = v > 0 ? v - 1 : 0;
    }
    if (v == 0) fault_at(small, PALACE_FASTG_ENONAME, s - 1);
    const bool pr = v > 0 && text[s + v - 1] == '\'';
    rec.name_len = v - (pr ? 1 : 0);
    name_recs[r] = rec;
    primed[r] = pr ? 1 : 0;
}

// the last record of (lo, hi] whose '>' is at or before pos, or lo when none is (lo: -1, or a record whose '>' is)
__device__ __forceinline__ int64_t record_at(const palace_fasta_rec *recs, int64_t lo, int64_t hi, int64_t pos)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (recs[mid].name_off - 1 <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kTileThreads) void fastg_check_kernel(const uint8_t *text, int64_t n, const palace_fasta_rec *recs, const uint8_t *primed,
                                                                   int64_t n_records, unsigned long long *small)
{
    __shared__ long long s_rec[2];
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTileBytes;
    if (threadIdx.x < 2) {
        const int64_t end = tile0 + kTileBytes < n ? tile0 + kTileBytes : n;
        s_rec[threadIdx.x] = record_at(recs, -1, n_records - 1, threadIdx.x == 0 ? tile0 : end - 1);
    }
    __syncthreads();
    const int64_t at = tile0 + threadIdx.x * kLaneBytes;
    if (at >= n) return;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    int64_t r = record_at(recs, s_rec[0], s_rec[1], at);
    int64_t next = r + 1 < n_records ? recs[r + 1].name_off - 1 : LLONG_MAX;
    int64_t seq = r >= 0 ? recs[r].seq_off : LLONG_MAX;
    bool pr = r >= 0 && primed[r];
    uint32_t prev = at > 0 ? text[at - 1] : '\n';
    int64_t bad_high = -1, bad_cr = -1, bad_plus = -1, bad_base = -1;        // the lane's first fault of each kind
#pragma unroll
    for (int k = 0; k < kLaneBytes; k++) {
        if (k < valid) {
            const int64_t p = at + k;
            const uint32_t c = byte_of(w, k);
            if (p >= next) {                                                 // the next record's '>'
                r++;
                seq = recs[r].seq_off; pr = primed[r];
                next = r + 1 < n_records ? recs[r + 1].name_off - 1 : LLONG_MAX;
            }
            if (r >= 0) {
                const uint32_t after = p + 1 < n ? (k + 1 < valid ? byte_of(w, (k + 1) & 15) : text[p + 1]) : 0u;
                if (p < seq) {                                               // a header line's byte
                    if (c >= 0x80u && bad_high < 0) bad_high = p;
                    if (c == '\r' && after != '\n' && bad_cr < 0) bad_cr = p;
                } else {
                    if (prev == '\n' && (c == '+' || c == '@') && bad_plus < 0) bad_plus = p;
                    if (pr && !is_base(c) && c != '\n' && !(c == '\r' && after == '\n') && bad_base < 0) bad_base = p;
                }
            }
            prev = c;
        }
    }
    if (bad_high >= 0) fault_at(small, PALACE_FASTG_EHIGH, bad_high);
    if (bad_cr >= 0) fault_at(small, PALACE_FASTG_ECR, bad_cr);
    if (bad_plus >= 0) fault_at(small, PALACE_FASTG_EPLUS, bad_plus);
    if (bad_base >= 0) fault_at(small, PALACE_FASTG_EBASE, bad_base);
    if (at + valid == n && prev != '\n') fault_at(small, PALACE_FASTG_ENOLF, n - 1);
}

// the line ends in front of each fault's offset
__global__ __launch_bounds__(kTileThreads) void fastg_fault_lines_kernel(const uint8_t *text, int64_t n, Offsets off, unsigned long long *small)
{
    const int64_t at = (static_cast<int64_t>(blockIdx.x) * kTileThreads + threadIdx.x) * kLaneBytes;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    const uint32_t nl = newline_mask(w, valid);
    for (int c = 0; c < kCodes; c++) {
        if (off.at[c] < 0) continue;                                         // (uniform)
        const int64_t left = off.at[c] - at;
        unsigned long long cnt = left <= 0 ? 0u : static_cast<unsigned>(__popc(left >= kLaneBytes ? nl : nl & ((1u << left) - 1u)));
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&small[kLinesAt + c], cnt);
    }
}

// ---- scans ----------------------------------------------------------------------------------------------------------------------

// bytes of record r in the output: '>' name LF sequence LF, nothing for a dropped record.  A name of no bytes is one the table
// of names never finds (its look-up refuses the empty name): of those the first record is kept here, and d_dup is put right.
struct OutSize {
    const palace_fasta_rec *recs;
    uint8_t *dup;
    const unsigned long long *small;
    __device__ __forceinline__ long long operator()(int64_t r) const
    {
        const palace_fasta_rec rec = recs[r];
        if (rec.name_len == 0) dup[r] = static_cast<unsigned long long>(r) != small[kFirstEmptyAt] ? 1 : 0;
        return dup[r] ? 0 : rec.name_len + rec.length + 3;
    }
};

__device__ __forceinline__ int digits_of(int64_t v)
{
    int d = 1;
    for (uint64_t x = static_cast<uint64_t>(v); x >= 10; x /= 10) d++;
    return d;
}

// bytes of record r's index row: name TAB length TAB offset TAB line_bases TAB line_width LF
struct RowSize {
    const palace_fasta_rec *recs;
    const uint8_t *skip;
    __device__ __forceinline__ long long operator()(int64_t r) const
    {
        if (skip && skip[r]) return 0;
        const palace_fasta_rec rec = recs[r];
        return rec.name_len + 5 + digits_of(rec.length) + digits_of(rec.seq_off) + digits_of(rec.line_bases) + digits_of(rec.line_width);
    }
};

__global__ __launch_bounds__(256) void first_empty_kernel(const palace_fasta_rec *recs, int64_t n_records, unsigned long long *small)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r < n_records && recs[r].name_len == 0) atomicMin(&small[kFirstEmptyAt], static_cast<unsigned long long>(r));
}

// the kept records as records of the output text, and how many they are
__global__ __launch_bounds__(256) void out_recs_kernel(const palace_fasta_rec *recs, const uint8_t *dup, const int64_t *out_off, int64_t n_records,
                                                       palace_fasta_rec *out_recs, unsigned long long *small)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool kept = r < n_records && !dup[r];
    if (r < n_records && out_recs) {
        const palace_fasta_rec rec = recs[r];
        const int64_t len = rec.length;
        out_recs[r] = palace_fasta_rec{rec.name_off, rec.name_len, out_off[r] + rec.name_len + 2, len, len, len ? len + 1 : 0};
    }
    const unsigned long long votes = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&small[kKeptAt], static_cast<unsigned long long>(__popcll(votes)));
}

// ---- the writer -------------------------------------------------------------------------------------------------------------------

// the items are the records; a primed one is read from its end through the upper-casing complement (window_lanes.hpp)
__global__ __launch_bounds__(kTileThreads) void fastg_write_kernel(const uint8_t *text, const palace_fasta_rec *recs, const uint8_t *primed,
                                                                   const int64_t *out_off, int64_t n_records, int64_t lo, int64_t hi, uint8_t *out)
{
    __shared__ long long s_rec[2];
    LaneOut l;
    int64_t r = window_lane(out_off, n_records, lo, hi, s_rec, &l);          // (behind dropped records it is the kept one)
    if (r < 0) return;
    while (!l.full() && r < n_records) {
        palace_fasta_rec rec = recs[r];
        if (rec.line_bases <= 0) rec.line_bases = 1;                         // (an indexed record with bases has a first line)
        const int64_t h = rec.name_len, len = rec.length;
        int64_t x = l.o0 + l.k - out_off[r];                                 // the byte's place in the record's text
        put_header(l, text + rec.name_off, h, x);
        if (l.full()) break;
        const int64_t q = x - (h + 2);                                       // ... in its sequence
        if (q < len) {
            const int64_t left = len - q;
            const int m = left < l.cnt - l.k ? static_cast<int>(left) : l.cnt - l.k;
            if (gather_bases(l, text, rec, q, m, primed[r] != 0, out, ComplementUpper())) return;
            if (l.full()) break;
        }
        l.put('\n');                                                         // the sequence's LF: the record is done
        r++;
        while (r < n_records && out_off[r + 1] == out_off[r]) r++;           // (dropped records)
    }
    l.store(out);
}

// ---- the index rows ---------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint8_t *put_number(uint8_t *p, int64_t v, uint8_t behind)
{
    const int d = digits_of(v);
    uint64_t x = static_cast<uint64_t>(v);
    for (int i = d - 1; i >= 0; i--) { p[i] = static_cast<uint8_t>('0' + x % 10); x /= 10; }
    p[d] = behind;
    return p + d + 1;
}

__global__ __launch_bounds__(256) void fai_rows_kernel(const uint8_t *text, const palace_fasta_rec *recs, const uint8_t *skip, int64_t n_records,
                                                       const int64_t *row_off, uint8_t *out)
{
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= n_records || (skip && skip[r])) return;
    const palace_fasta_rec rec = recs[r];
    uint8_t *p = out + row_off[r];
    for (int64_t i = 0; i < rec.name_len; i++) p[i] = text[rec.name_off + i];
    p += rec.name_len;
    *p++ = '\t';
    p = put_number(p, rec.length, '\t');
    p = put_number(p, rec.seq_off, '\t');
    p = put_number(p, rec.line_bases, '\t');
    put_number(p, rec.line_width, '\n');
}

inline unsigned blocks_of(int64_t n, int per) { return static_cast<unsigned>((n + per - 1) / per); }

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_fastg_derive(palace_ctx *ctx, const uint8_t *d_text, int64_t n, const palace_fasta_rec *d_recs, int64_t n_records,
                                   palace_fasta_rec *d_name_recs, uint8_t *d_primed, palace_fasta_status *status_out)
{
    PALACE_REQUIRE(ctx && n >= 0 && n_records >= 0 && n_records < (1ll << 29) && status_out, "bad argument (at most 2^29 - 1 records)");
    PALACE_REQUIRE((d_text || n == 0) && (n_records == 0 || (d_recs && d_name_recs && d_primed)), "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15) == 0, "the text must be 16-byte aligned");
    const int64_t nt = (n + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE(nt < (1ll << 31), "text too long");
    *status_out = palace_fasta_status{n_records, 0, 0, 0};
    if (n == 0) { status_out->bad_line = 1; status_out->error = PALACE_FASTG_EEMPTY; return PALACE_OK; }
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    PALACE_HIP_TRY(hipMemsetAsync(small + kOffAt, 0xff, kCodes * sizeof(unsigned long long), ctx->stream));
    PALACE_HIP_TRY(hipMemsetAsync(small + kLinesAt, 0, kCodes * sizeof(unsigned long long), ctx->stream));
    if (n_records)
        hipLaunchKernelGGL(fastg_names_kernel, dim3(blocks_of(n_records, 256)), dim3(256), 0, ctx->stream, d_text, n, d_recs, n_records, d_name_recs, d_primed,
                           small);
    hipLaunchKernelGGL(fastg_check_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, n, d_recs, d_primed, n_records, small);
    PALACE_HIP_TRY(hipGetLastError());
    unsigned long long off[kCodes], lines[kCodes];
    PALACE_HIP_TRY(hipMemcpyAsync(off, small + kOffAt, sizeof off, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    Offsets o;
    int64_t far = -1;
    for (int c = 0; c < kCodes; c++) {
        o.at[c] = off[c] == ~0ull ? -1 : static_cast<long long>(off[c]);
        if (o.at[c] > far) far = o.at[c];
    }
    if (far < 0) return PALACE_OK;
    if (far > 0)                                                             // (a fault in the first byte has no line end in front of it)
        hipLaunchKernelGGL(fastg_fault_lines_kernel, dim3(blocks_of(far, kTileBytes)), dim3(kTileThreads), 0, ctx->stream, d_text, far, o, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(lines, small + kLinesAt, sizeof lines, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int c = kCodes - 1; c >= 0; c--) {
        if (o.at[c] < 0) continue;
        const int64_t line = static_cast<int64_t>(lines[c]) + 1;
        if (status_out->error == 0 || line <= status_out->bad_line) { status_out->bad_line = line; status_out->error = c; }
    }
    return PALACE_OK;
}

extern "C" int palace_fastg_plan(palace_ctx *ctx, const palace_fasta_rec *d_name_recs, uint8_t *d_dup, int64_t n_records, int64_t *d_out_off,
                                 palace_fasta_rec *d_out_recs, int64_t *n_kept_out, int64_t *out_bytes_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 29) && d_out_off && n_kept_out && out_bytes_out, "bad argument");
    PALACE_REQUIRE(n_records == 0 || (d_name_recs && d_dup), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    *n_kept_out = *out_bytes_out = 0;
    if (n_records == 0) { PALACE_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(int64_t), ctx->stream)); return PALACE_OK; }
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    PALACE_HIP_TRY(hipMemsetAsync(small + kFirstEmptyAt, 0xff, sizeof(unsigned long long), ctx->stream));
    PALACE_HIP_TRY(hipMemsetAsync(small + kKeptAt, 0, sizeof(unsigned long long), ctx->stream));
    const dim3 grid(blocks_of(n_records, 256));
    hipLaunchKernelGGL(first_empty_kernel, grid, dim3(256), 0, ctx->stream, d_name_recs, n_records, small);
    const int rc = scan_sizes(ctx, OutSize{d_name_recs, d_dup, small}, n_records, d_out_off);
    if (rc) return rc;
    hipLaunchKernelGGL(out_recs_kernel, grid, dim3(256), 0, ctx->stream, d_name_recs, d_dup, d_out_off, n_records, d_out_recs, small);
    PALACE_HIP_TRY(hipGetLastError());
    unsigned long long kept = 0;
    int64_t total = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&kept, small + kKeptAt, sizeof kept, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(&total, d_out_off + n_records, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_kept_out = static_cast<int64_t>(kept);
    *out_bytes_out = total;
    return PALACE_OK;
}

extern "C" int palace_fastg_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_name_recs, const uint8_t *d_primed,
                                  const int64_t *d_out_off, int64_t n_records, int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && lo >= 0 && lo <= hi, "bad argument");
    if (lo == hi) return PALACE_OK;
    PALACE_REQUIRE(n_records > 0 && d_text && d_name_recs && d_primed && d_out_off && d_out, "null device pointer (or bytes asked of an empty text)");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (hi - lo + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE(nt < (1ll << 31), "window too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(fastg_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, d_name_recs, d_primed, d_out_off,
                       n_records, lo, hi, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_fai_rows_plan(palace_ctx *ctx, const palace_fasta_rec *d_recs, const uint8_t *d_skip, int64_t n_records, int64_t *d_row_off,
                                    int64_t *bytes_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 29) && d_row_off && bytes_out, "bad argument");
    PALACE_REQUIRE(n_records == 0 || d_recs, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    *bytes_out = 0;
    if (n_records == 0) { PALACE_HIP_TRY(hipMemsetAsync(d_row_off, 0, sizeof(int64_t), ctx->stream)); return PALACE_OK; }
    const int rc = scan_sizes(ctx, RowSize{d_recs, d_skip}, n_records, d_row_off);
    if (rc) return rc;
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(bytes_out, d_row_off + n_records, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PALACE_OK;
}

extern "C" int palace_fai_rows_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const uint8_t *d_skip, int64_t n_records,
                                     const int64_t *d_row_off, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0, "bad argument");
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_text && d_recs && d_row_off && d_out, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(fai_rows_kernel, dim3(blocks_of(n_records, 256)), dim3(256), 0, ctx->stream, d_text, d_recs, d_skip, n_records, d_row_off, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
