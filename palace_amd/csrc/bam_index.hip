// bamsort's index half (the driver's `samtools index`, palace:433): the arithmetic of a .bai (SAM specification 5.2) on
// a coordinate-sorted stream where it lies -- what each record is filed under (bam_record.hpp: bai_span, reg2bin), the chunks as runs
// of equal (refID, bin) ordered with palace_sort_u64, the 16 kb linear index and the pseudo-bin's numbers per reference, and the map
// from stream offsets to BGZF virtual offsets.  The host lays the arrays out as the file's bytes (host/bai.hpp).
#include "common.hpp"
#include "bam_record.hpp"
#include "scan64.hpp"

namespace palace {
namespace {


// small[0] = records a .bai cannot hold, [1] = the first of them, [2] = the first record out of order, [3] = records without a contig
__global__ __launch_bounds__(256) void bai_records_kernel(const uint8_t *stream, const int64_t *starts, int64_t n, int32_t n_ref, int32_t *ref, int32_t *bin,
                                                          int32_t *win_beg, int32_t *win_end, uint8_t *unmapped, unsigned long long *small)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const bool valid = i < n;
    bool no_coor = false;
    if (valid) {
        const int64_t s = starts[i];
        const int32_t tid = static_cast<int32_t>(ld32(stream, s));
        const uint32_t flag = ld16(stream, s + 14);
        int32_t r = -1, b = 0, wb = 0, we = 0;
        bool bad = tid < -1 || tid >= n_ref;
        if (tid == -1) no_coor = true;
        else if (!bad) {
            const BaiSpan sp = bai_span(stream, s);
            if (!sp.ok) bad = true;
            else {
                r = tid;
                b = static_cast<int32_t>(reg2bin(sp.beg, sp.end));
                wb = static_cast<int32_t>(sp.beg >> 14);
                we = static_cast<int32_t>((sp.end - 1) >> 14);
            }
        }
        if (bad) {
            atomicAdd(&small[0], 1ull);
            atomicMin(&small[1], static_cast<unsigned long long>(i));
        }
        if (i > 0) {
            const int64_t p = starts[i - 1];
            if (sort_key_ok(stream, s, n_ref) && sort_key_ok(stream, p, n_ref) && sort_key(stream, s, n_ref) < sort_key(stream, p, n_ref))
                atomicMin(&small[2], static_cast<unsigned long long>(i));
        }
        ref[i] = r; bin[i] = b; win_beg[i] = wb; win_end[i] = we; unmapped[i] = (flag & 4u) ? 1 : 0;
    }
    const unsigned long long m = __ballot(no_coor);                        // one add per wave for the unplaced tail
    if (no_coor && (threadIdx.x & 63) == __ffsll(static_cast<long long>(m)) - 1) atomicAdd(&small[3], static_cast<unsigned long long>(__popcll(m)));
}

__device__ __forceinline__ bool run_head(const int32_t *ref, const int32_t *bin, int64_t i) { return i == 0 || ref[i] != ref[i - 1] || bin[i] != bin[i - 1]; }

__global__ __launch_bounds__(kScanThreads) void bai_head_scan_kernel(const int32_t *ref, const int32_t *bin, int64_t n, int64_t *cum, long long *sums)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    const long long v = i < n && run_head(ref, bin, i) ? 1 : 0;
    long long total;
    const long long ex = block_exclusive<long long, kScanThreads>(v, s_scan, &total);
    if (i < n) cum[i] = ex;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// run c: its first record, and its key (refID, bin) with the unplaced records' runs behind every reference
__global__ __launch_bounds__(256) void bai_heads_kernel(const int32_t *ref, const int32_t *bin, int64_t n, int32_t n_ref, const int64_t *cum, int64_t cap,
                                                        uint32_t *head, uint64_t *key)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n || !run_head(ref, bin, i)) return;
    const int64_t c = cum[i];
    if (c >= cap) return;
    head[c] = static_cast<uint32_t>(i);
    key[c] = static_cast<uint64_t>(static_cast<uint32_t>(ref[i] < 0 ? n_ref : ref[i])) << 16 | static_cast<uint32_t>(bin[i]);
}

__global__ __launch_bounds__(256) void bai_chunks_kernel(const uint8_t *stream, const int64_t *starts, const int32_t *ref, const int32_t *bin, int64_t n,
                                                         const uint32_t *head, const uint32_t *perm, int64_t n_runs, int32_t *c_ref, int32_t *c_bin, int64_t *c_beg,
                                                         int64_t *c_end)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n_runs) return;
    const int64_t c = perm[k], i0 = head[c], i1 = (c + 1 < n_runs ? static_cast<int64_t>(head[c + 1]) : n) - 1;
    c_ref[k] = ref[i0];
    c_bin[k] = bin[i0];
    c_beg[k] = starts[i0] - 4;
    c_end[k] = starts[i1] + static_cast<int64_t>(ld32(stream, starts[i1] - 4));
}

constexpr unsigned long long kNone = ~0ull;
constexpr int kStrip = 16;                          // consecutive records a lane folds before it touches memory (a deep reference is one address)

__global__ __launch_bounds__(256) void bai_ref_init_kernel(int32_t n_ref, int32_t *n_intv, unsigned long long *stat)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n_ref) return;
    n_intv[t] = 0;
    stat[t] = 0; stat[n_ref + t] = 0; stat[2ll * n_ref + t] = kNone; stat[3ll * n_ref + t] = 0;
}

__global__ __launch_bounds__(256) void bai_ref_stat_kernel(const uint8_t *stream, const int64_t *starts, const int32_t *ref, const int32_t *win_end,
                                                           const uint8_t *unmapped, int64_t n, int32_t n_ref, int32_t *n_intv, unsigned long long *stat)
{
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * kStrip, i1 = i0 + kStrip < n ? i0 + kStrip : n;
    int32_t cur = -1, hi = 0;
    unsigned long long n_map = 0, n_un = 0, first = kNone, last = 0;
    auto flush = [&] {
        if (cur < 0) return;
        atomicMax(&n_intv[cur], hi + 1);
        if (n_map) atomicAdd(&stat[cur], n_map);
        if (n_un) atomicAdd(&stat[n_ref + cur], n_un);
        atomicMin(&stat[2ll * n_ref + cur], first);
        atomicMax(&stat[3ll * n_ref + cur], last);
    };
    for (int64_t i = i0; i < i1; i++) {
        const int32_t r = ref[i];
        if (r != cur) { flush(); cur = r; hi = 0; n_map = n_un = 0; first = kNone; last = 0; }
        if (r < 0) continue;
        const int64_t s = starts[i];
        const unsigned long long beg = static_cast<unsigned long long>(s - 4), end = static_cast<unsigned long long>(s + static_cast<int64_t>(ld32(stream, s - 4)));
        hi = win_end[i] > hi ? win_end[i] : hi;
        if (unmapped[i]) n_un++; else n_map++;
        first = beg < first ? beg : first;
        last = end > last ? end : last;
    }
    flush();
}

// the file is sorted: of a lane's records the first that reaches a window has the smallest start, so a window below the highest one
// the lane has already written for this reference needs no second look
__global__ __launch_bounds__(256) void bai_linear_kernel(const int64_t *starts, const int32_t *ref, const int32_t *win_beg, const int32_t *win_end, int64_t n,
                                                         const int64_t *lin_off, int64_t n_lin, unsigned long long *lin)
{
    const int64_t i0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * kStrip, i1 = i0 + kStrip < n ? i0 + kStrip : n;
    int32_t cur = -1, done = -1;
    for (int64_t i = i0; i < i1; i++) {
        const int32_t r = ref[i];
        if (r < 0) continue;
        if (r != cur) { cur = r; done = -1; }
        const int64_t base = lin_off[r], room = lin_off[r + 1] - base;
        const int32_t wb = win_beg[i] > done + 1 ? win_beg[i] : done + 1;
        for (int32_t w = wb; w <= win_end[i] && w < room && base + w < n_lin; w++) atomicMin(&lin[base + w], static_cast<unsigned long long>(starts[i] - 4));
        done = win_end[i] > done ? win_end[i] : done;
    }
}

__global__ __launch_bounds__(256) void bai_linear_fill_kernel(int32_t n_ref, const int64_t *lin_off, int64_t n_lin, unsigned long long *lin)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n_ref) return;
    unsigned long long v = kNone;
    for (int64_t w = (lin_off[t + 1] < n_lin ? lin_off[t + 1] : n_lin) - 1; w >= lin_off[t] && w >= 0; w--) {
        if (lin[w] == kNone) lin[w] = v; else v = lin[w];
    }
}

__global__ __launch_bounds__(256) void bgzf_voffsets_kernel(const int64_t *u, int64_t n, const int64_t *mem_u, const int64_t *mem_c, int64_t n_members, uint64_t *voff)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t v = u[k];
    if (v < mem_u[0] || v > mem_u[n_members - 1]) { voff[k] = ~0ull; return; }
    const int64_t m = last_le(mem_u, 0, n_members - 1, v);
    voff[k] = static_cast<uint64_t>(mem_c[m]) << 16 | static_cast<uint64_t>(v - mem_u[m]);
}

int bits_of(uint32_t v) { int b = 0; while (v) { b++; v >>= 1; } return b; }

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_bai_records(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, int64_t n_records, int32_t n_ref, int32_t *d_ref,
                                  int32_t *d_bin, int32_t *d_win_beg, int32_t *d_win_end, uint8_t *d_unmapped, palace_bai_status *status_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && n_ref >= 0 && status_out, "bad argument");
    PALACE_REQUIRE(n_records == 0 || (d_stream && d_starts && d_ref && d_bin && d_win_beg && d_win_end && d_unmapped), "null device pointer");
    *status_out = palace_bai_status{0, -1, -1, 0};
    if (n_records == 0) return PALACE_OK;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    const unsigned long long init[4] = {0, ~0ull, ~0ull, 0};
    unsigned long long got[4];
    PALACE_HIP_TRY(hipMemcpyAsync(small, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (init is this call's own)
    hipLaunchKernelGGL(bai_records_kernel, dim3(static_cast<unsigned>((n_records + 255) / 256)), dim3(256), 0, ctx->stream, d_stream, d_starts, n_records, n_ref,
                       d_ref, d_bin, d_win_beg, d_win_end, d_unmapped, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(got, small, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    status_out->n_bad = static_cast<int64_t>(got[0]);
    status_out->first_bad = got[0] ? static_cast<int64_t>(got[1]) : -1;
    status_out->first_unsorted = got[2] == ~0ull ? -1 : static_cast<int64_t>(got[2]);
    status_out->n_no_coor = static_cast<int64_t>(got[3]);
    return PALACE_OK;
}

extern "C" int palace_bai_chunks(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const int32_t *d_ref, const int32_t *d_bin,
                                 int64_t n_records, int32_t n_ref, int32_t *d_chunk_ref, int32_t *d_chunk_bin, int64_t *d_chunk_beg, int64_t *d_chunk_end,
                                 int64_t cap, int64_t *n_runs_out)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && n_ref >= 0 && cap >= 0 && cap < (1ll << 31) && n_runs_out, "bad argument");
    *n_runs_out = 0;
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts && d_ref && d_bin, "null device pointer");
    const bool write = d_chunk_ref && d_chunk_bin && d_chunk_beg && d_chunk_end && cap > 0;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    // the workspace: block sums, the scan, and -- sized by cap -- run heads, keys, permutation and the sort's scratch
    const int64_t nb = (n_records + kScanThreads - 1) / kScanThreads;
    const size_t b_sums = align256(static_cast<size_t>(nb + 1) * 8), b_cum = align256(static_cast<size_t>(n_records + 1) * 8);
    const size_t b_head = write ? align256(static_cast<size_t>(cap) * 4) : 0, b_key = write ? align256(static_cast<size_t>(cap) * 8) : 0;
    const size_t b_sort = write ? palace_sort_u64_scratch_bytes(cap) : 0;
    const int rc = ensure_workspace(ctx, b_sums + b_cum + 2 * b_head + b_key + b_sort + 256);
    if (rc) return rc;
    uint8_t *w = reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(ctx->ws.ptr) + 255) & ~static_cast<uintptr_t>(255));
    long long *sums = reinterpret_cast<long long *>(w);
    int64_t *cum = reinterpret_cast<int64_t *>(w + b_sums);
    uint32_t *head = reinterpret_cast<uint32_t *>(w + b_sums + b_cum), *perm = reinterpret_cast<uint32_t *>(w + b_sums + b_cum + b_head);
    uint64_t *key = reinterpret_cast<uint64_t *>(w + b_sums + b_cum + 2 * b_head);
    void *sort_scratch = w + b_sums + b_cum + 2 * b_head + b_key;
    hipLaunchKernelGGL(bai_head_scan_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, d_ref, d_bin, n_records, cum, sums);
    hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
    hipLaunchKernelGGL(add_block_base_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, n_records, cum, sums, nb);
    PALACE_HIP_TRY(hipGetLastError());
    int64_t n_runs = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&n_runs, cum + n_records, sizeof n_runs, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_runs_out = n_runs;
    if (!write || cap < n_runs) return PALACE_OK;
    hipLaunchKernelGGL(bai_heads_kernel, dim3(static_cast<unsigned>((n_records + 255) / 256)), dim3(256), 0, ctx->stream, d_ref, d_bin, n_records, n_ref, cum, n_runs,
                       head, key);
    PALACE_HIP_TRY(hipGetLastError());
    const int rs = palace_sort_u64(ctx, key, perm, n_runs, 16 + bits_of(static_cast<uint32_t>(n_ref)), sort_scratch, b_sort);
    if (rs) return rs;
    hipLaunchKernelGGL(bai_chunks_kernel, dim3(static_cast<unsigned>((n_runs + 255) / 256)), dim3(256), 0, ctx->stream, d_stream, d_starts, d_ref, d_bin, n_records,
                       head, perm, n_runs, d_chunk_ref, d_chunk_bin, d_chunk_beg, d_chunk_end);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (the workspace is the next call's again)
    return PALACE_OK;
}

extern "C" int palace_bai_linear(palace_ctx *ctx, const uint8_t *d_stream, const int64_t *d_starts, const int32_t *d_ref, const int32_t *d_win_beg,
                                 const int32_t *d_win_end, const uint8_t *d_unmapped, int64_t n_records, int32_t n_ref, int32_t *d_n_intv,
                                 int64_t *d_ref_stat, const int64_t *d_lin_off, int64_t n_lin, int64_t *d_lin)
{
    PALACE_REQUIRE(ctx && n_records >= 0 && n_records < (1ll << 31) && n_ref >= 0, "bad argument");
    if (n_ref == 0) return PALACE_OK;
    PALACE_REQUIRE(n_records == 0 || (d_stream && d_starts && d_ref && d_win_beg && d_win_end && d_unmapped), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const dim3 refs(static_cast<unsigned>((static_cast<int64_t>(n_ref) + 255) / 256)), strips(static_cast<unsigned>((n_records + 256 * kStrip - 1) / (256 * kStrip)));
    if (!d_lin) {
        PALACE_REQUIRE(d_n_intv && d_ref_stat, "null device pointer");
        unsigned long long *stat = reinterpret_cast<unsigned long long *>(d_ref_stat);
        hipLaunchKernelGGL(bai_ref_init_kernel, refs, dim3(256), 0, ctx->stream, n_ref, d_n_intv, stat);
        if (n_records)
            hipLaunchKernelGGL(bai_ref_stat_kernel, strips, dim3(256), 0, ctx->stream, d_stream, d_starts, d_ref, d_win_end, d_unmapped, n_records, n_ref, d_n_intv, stat);
    } else {
        PALACE_REQUIRE(d_lin_off && n_lin >= 0, "null device pointer");
        unsigned long long *lin = reinterpret_cast<unsigned long long *>(d_lin);
        PALACE_HIP_TRY(hipMemsetAsync(d_lin, 0xff, static_cast<size_t>(n_lin) * 8, ctx->stream));
        if (n_records) hipLaunchKernelGGL(bai_linear_kernel, strips, dim3(256), 0, ctx->stream, d_starts, d_ref, d_win_beg, d_win_end, n_records, d_lin_off, n_lin, lin);
        hipLaunchKernelGGL(bai_linear_fill_kernel, refs, dim3(256), 0, ctx->stream, n_ref, d_lin_off, n_lin, lin);
    }
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bgzf_voffsets(palace_ctx *ctx, const int64_t *d_u, int64_t n, const int64_t *d_member_u, const int64_t *d_member_c, int64_t n_members,
                                    uint64_t *d_voff)
{
    PALACE_REQUIRE(ctx && n >= 0 && n_members >= 1, "bad argument (at least one member entry)");
    if (n == 0) return PALACE_OK;
    PALACE_REQUIRE(d_u && d_member_u && d_member_c && d_voff, "null device pointer");
    PALACE_REQUIRE(n < (1ll << 39), "too many offsets");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bgzf_voffsets_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream, d_u, n, d_member_u, d_member_c, n_members, d_voff);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
