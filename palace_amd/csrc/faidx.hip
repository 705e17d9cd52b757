// `samtools faidx <file.fa> region ...` on the device (include/palace_hip.h: palace_faidx_resolve .. palace_faidx_write): regions
// -> records and ranges, the output's layout, and any window of the output text.  The rules: DESIGN.md 8; the grammar of a region:
// faidx_region.hpp.  The text is indexed by palace_fasta_index and its names hashed by palace_fasta_names_create (path_fasta.hip).
//   resolve: one lane per region; the look-ups are the name table's.
//   plan:    a 64-bit scan of the regions' output sizes (a failed region has none; scan64.hpp); the smallest failed region is
//            reduced beside it.
//   write:   any window [lo, hi) of the output, by the lanes and the gather of window_lanes.hpp: the items are the regions.  A
//            region's text is '>' header LF and its bases in lines of line_len, every line ended by LF -- the output's line grid
//            and the record's do not line up, so a lane's run of bases ends where either line ends: 16 neighbours of one output
//            line and one source line are one load and one store, everything else is walked.
#include "common.hpp"
#include "faidx_region.hpp"
#include "fasta_names.hpp"
#include "window_lanes.hpp"

namespace palace {
namespace {

static_assert(sizeof(palace_faidx_region) == 24 && sizeof(FaidxRegion) == sizeof(palace_faidx_region), "region layout");

constexpr int kFirstFailedAt = 0;                // ctx->d_small, in 64-bit words: the smallest failed region

__global__ __launch_bounds__(256) void faidx_resolve_kernel(palace_fasta_names t, const palace_fasta_rec *recs, const uint8_t *reg, const int64_t *off,
                                                            int64_t n_regions, palace_faidx_region *out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_regions) return;
    const FaidxRegion g = faidx_region_resolve(
        reg + off[i], off[i + 1] - off[i], [&t](const uint8_t *p, int64_t n) { return static_cast<int64_t>(record_of(t, p, n)); },
        [recs](int64_t r) { return recs[r].length; });
    out[i] = palace_faidx_region{g.rec, g.beg, g.len};
}

// bytes of region i in the output: '>' header LF, its bases and an LF behind every line; nothing for a failed region
struct RegionSize {
    const palace_faidx_region *regs;
    const int64_t *hdr_off;
    int64_t line_len;
    unsigned long long *small;
    __device__ __forceinline__ long long operator()(int64_t i) const
    {
        const palace_faidx_region g = regs[i];
        if (g.rec < 0) { atomicMin(&small[kFirstFailedAt], static_cast<unsigned long long>(i)); return 0; }
        return 2 + (hdr_off[i + 1] - hdr_off[i]) + g.len + (g.len + line_len - 1) / line_len;
    }
};

__global__ __launch_bounds__(kTileThreads) void faidx_write_kernel(const uint8_t *text, const palace_fasta_rec *recs, const palace_faidx_region *regs,
                                                                   int64_t n_regions, const uint8_t *hdr, const int64_t *hdr_off, const int64_t *out_off,
                                                                   int64_t line_len, bool rev, int64_t lo, int64_t hi, uint8_t *out)
{
    __shared__ long long s_reg[2];
    LaneOut l;
    int64_t p = window_lane(out_off, n_regions, lo, hi, s_reg, &l);          // (behind regions without text it is the one with text)
    if (p < 0) return;
    const int64_t row_bytes = line_len + 1;
    while (!l.full() && p < n_regions) {
        const palace_faidx_region g = regs[p];
        const int64_t h0 = hdr_off[p], h = hdr_off[p + 1] - h0, body = g.len + (g.len + line_len - 1) / line_len;
        int64_t x = l.o0 + l.k - out_off[p];                                 // the byte's place in the region's text
        put_header(l, hdr + h0, h, x);
        if (l.full()) break;
        int64_t y = x - (h + 2);                                             // ... in its body
        if (y < body) {
            const palace_fasta_rec r = recs[g.rec];
            int64_t row = y / row_bytes, col = y - row * row_bytes;
            while (!l.full() && y < body) {
                const int64_t q = row * line_len + col;                      // ... among its bases
                if (col == line_len || q == g.len) {                         // a line's LF; the last line may be shorter
                    l.put('\n');
                    y++; row++; col = 0;
                    continue;
                }
                const int64_t in_line = line_len - col, in_all = g.len - q, left = in_line < in_all ? in_line : in_all;
                const int m = left < l.cnt - l.k ? static_cast<int>(left) : l.cnt - l.k;
                if (gather_bases(l, text, r, g.beg, g.len, q, m, rev, out, ComplementAmbiguous())) return;
                y += m; col += m;
            }
            if (l.full()) break;
        }
        p++;
        while (p < n_regions && out_off[p + 1] == out_off[p]) p++;           // (failed regions)
    }
    l.store(out);
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_faidx_resolve(palace_ctx *ctx, const palace_fasta_names *names, const palace_fasta_rec *d_recs, const uint8_t *d_reg,
                                    const int64_t *d_reg_off, int64_t n_regions, palace_faidx_region *d_out)
{
    PALACE_REQUIRE(ctx && names && n_regions >= 0 && n_regions < (1ll << 39), "bad argument");
    if (n_regions == 0) return PALACE_OK;
    PALACE_REQUIRE(d_reg_off && d_out && (d_recs || names->n == 0), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(faidx_resolve_kernel, dim3(static_cast<unsigned>((n_regions + 255) / 256)), dim3(256), 0, ctx->stream, *names, d_recs, d_reg, d_reg_off,
                       n_regions, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_faidx_plan(palace_ctx *ctx, const palace_faidx_region *d_regions, int64_t n_regions, const int64_t *d_hdr_off, int64_t line_len,
                                 int skip_failed, int64_t *d_out_off, int64_t *total_out, int64_t *first_failed_out)
{
    PALACE_REQUIRE(ctx && n_regions >= 0 && n_regions < (1ll << 39) && line_len >= 1 && d_out_off && total_out && first_failed_out, "bad argument");
    PALACE_REQUIRE(n_regions == 0 || (d_regions && d_hdr_off), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    *total_out = 0;
    *first_failed_out = -1;
    if (n_regions == 0) {
        PALACE_HIP_TRY(hipMemsetAsync(d_out_off, 0, sizeof(int64_t), ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return PALACE_OK;
    }
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    PALACE_HIP_TRY(hipMemsetAsync(small + kFirstFailedAt, 0xff, sizeof(unsigned long long), ctx->stream));
    const int rc = scan_sizes(ctx, RegionSize{d_regions, d_hdr_off, line_len, small}, n_regions, d_out_off);
    if (rc) return rc;
    PALACE_HIP_TRY(hipGetLastError());
    unsigned long long first = 0;
    int64_t total = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&first, small + kFirstFailedAt, sizeof first, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(&total, d_out_off + n_regions, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *first_failed_out = first == ~0ull ? -1 : static_cast<int64_t>(first);
    if (*first_failed_out >= 0 && !skip_failed) {                            // nothing is written then: a text of no bytes
        PALACE_HIP_TRY(hipMemsetAsync(d_out_off, 0, static_cast<size_t>(n_regions + 1) * sizeof(int64_t), ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
        total = 0;
    }
    *total_out = total;
    return PALACE_OK;
}

extern "C" int palace_faidx_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const palace_faidx_region *d_regions,
                                  int64_t n_regions, const uint8_t *d_hdr, const int64_t *d_hdr_off, const int64_t *d_out_off, int64_t line_len,
                                  int reverse, int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_regions >= 0 && line_len >= 1 && lo >= 0 && lo <= hi, "bad argument");
    if (lo == hi) return PALACE_OK;
    PALACE_REQUIRE(n_regions > 0 && d_regions && d_hdr_off && d_out_off && d_out, "null device pointer (or bytes asked of an empty text)");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (hi - lo + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE(nt < (1ll << 31), "window too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(faidx_write_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, d_recs, d_regions, n_regions, d_hdr,
                       d_hdr_off, d_out_off, line_len, reverse != 0, lo, hi, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
