// samview's device half (the driver's `samtools view -buS`, palace:421-423): the lines of a SAM text where it lies
// (palace_sam_lines), every alignment line validated and sized (palace_sam_plan), and the BAM records written at the scanned
// offsets (palace_sam_encode).  What a line MEANS is sam_line.hpp's; this file is who reads which byte.
//
// The lines.  Every workgroup counts the LFs of its tile of T = 4096 bytes (a lane's 16 bytes, text_lanes.hpp), one workgroup scans
// the tiles' counts, the tiles are taken again and every LF in front of the text's last byte writes the start behind it.
//
// A line.  A wavefront owns a line, four lines to a workgroup: nothing is shared between them, so no workgroup barrier is met
// and a short line's wave is done when it is done.  The lanes take the line 64 bytes at a time; the TABs of a stretch are one ballot,
// a TAB's ordinal the set bits below it, and the first eleven cuts go to the wave's 12 words of LDS, from where every lane reads all
// of them.  The eight numeric fields and the two look-ups are done by every lane alike (the loads are one address per wave).  The
// CIGAR is taken a byte per lane: the lane of an op's letter walks back over its digits, its ordinal is again a ballot.  QUAL is
// checked, SEQ packed and QUAL shifted a byte of output per lane.  The tags are found by ballot 64 at a time and parsed a tag per
// lane, their places are a wave scan of their sizes, and the text of a Z / H value is copied by all lanes.  The plan and the encode
// are ONE function (kEncode adds the stores), so the size a record was given is the size it takes.
#include "common.hpp"
#include "sam_line.hpp"
#include "bam_names.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"     // (scan64.hpp's add_block_base_kernel and last_le are not used here)
#include "scan64.hpp"
#pragma clang diagnostic pop

namespace palace {
namespace {

constexpr int kLineThreads = 256, kLineTile = PALACE_SAM_TILE;
static_assert(kLineThreads * kLaneBytes == kLineTile, "a lane takes 16 bytes of the tile");
constexpr int64_t kMaxLine = 1ll << 29;


// the lane's LFs that begin a line: every LF but one that is the text's last byte
__device__ __forceinline__ uint32_t line_lf_mask(const uint8_t *text, int64_t n, int64_t at)
{
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    uint32_t m = newline_mask(w, valid);
    const int64_t last = n - 1 - at;
    if (last >= 0 && last < kLaneBytes) m &= ~(1u << last);
    return m;
}

__global__ __launch_bounds__(kLineThreads) void sam_count_kernel(const uint8_t *text, int64_t n, long long *tile_count)
{
    __shared__ long long lds[kLineThreads / 64 + 1];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kLineTile + threadIdx.x * kLaneBytes;
    long long total;
    block_exclusive<long long, kLineThreads>(__popc(line_lf_mask(text, n, at)), lds, &total);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

// tile_base: the exclusive sums of the tiles' counts; line 0 begins at 0, line k >= 1 behind the k-th counted LF
__global__ __launch_bounds__(kLineThreads) void sam_scatter_kernel(const uint8_t *text, int64_t n, const long long *tile_base, int64_t n_lines, int64_t *start)
{
    __shared__ long long lds[kLineThreads / 64 + 1];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kLineTile + threadIdx.x * kLaneBytes;
    uint32_t m = line_lf_mask(text, n, at);
    long long total;
    int64_t ord = 1 + tile_base[blockIdx.x] + block_exclusive<long long, kLineThreads>(__popc(m), lds, &total);
    for (; m; m &= m - 1, ord++)
        if (ord < n_lines) start[ord] = at + __ffs(static_cast<int>(m));     // (ord < n_lines always: the counts are those of these bytes)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        start[0] = 0;
        start[n_lines] = n + (text[n - 1] != '\n' ? 1 : 0);
    }
}

// small[0] = the first line that is empty or does not begin with '@'
__global__ __launch_bounds__(256) void sam_first_kernel(const uint8_t *text, const int64_t *start, int64_t n_lines, unsigned long long *small)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n_lines) return;
    const int64_t b = start[k], e = start[k + 1] - 1;
    if (e == b || text[b] != '@') atomicMin(&small[0], static_cast<unsigned long long>(k));
}
// small[1] = the smallest (line number << 8 | code) of the lines' own faults, small[2] = a line is longer than kMaxLine
__global__ __launch_bounds__(256) void sam_lines_err_kernel(const uint8_t *text, const int64_t *start, int64_t n_lines, unsigned long long *small)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (k >= n_lines) return;
    const int64_t b = start[k], e = start[k + 1] - 1;
    int code = 0;
    if (e == b) code = PALACE_SAM_EEMPTY;
    else if (text[b] == '@' && static_cast<unsigned long long>(k) > small[0]) code = PALACE_SAM_EAT;
    if (code) atomicMin(&small[1], static_cast<unsigned long long>(k + 1) << 8 | static_cast<unsigned long long>(code));
    if (e - b > kMaxLine) small[2] = 1;
}

// ---- one line, one wavefront -----------------------------------------------------------------------------------------------------

constexpr int kSamThreads = 256, kSamWaves = kSamThreads / kWave, kTagBatch = 64;
struct WaveCuts { int64_t c[12]; int64_t tag[kTagBatch + 1]; };

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ long long wave_sum(long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ long long wave_exclusive(long long v, int lane)
{
    long long inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    return inc - v;
}

// The line [b, e): *code_out its first error, *size_out its record's bytes (0: an error, or the mask drops it); kEncode: the record
// goes to o + at (for a line the plan kept: mask 0).  The steps and their order are sam_line's (sam_line.hpp).
template <bool kEncode>
__device__ __forceinline__ void sam_line_wave(const uint8_t *t, int64_t b, int64_t e, const palace_bam_names &names, uint32_t mask, volatile WaveCuts *L,
                                              int lane, int32_t *code_out, int64_t *size_out, uint8_t *o, int64_t at)
{
    *size_out = 0;
    // the cut
    if (lane == 0) L->c[0] = b;
    int64_t tabs = 0;
    for (int64_t p = b; p < e && tabs < 11; p += kWave) {
        const int64_t q = p + lane;
        const bool tab = q < e && t[q] == '\t';
        const unsigned long long m = __ballot(tab);
        if (tab) {
            const int64_t ord = tabs + __popcll(m & lanes_below(lane));
            if (ord < 11) L->c[ord + 1] = q + 1;
        }
        tabs += __popcll(m);
    }
    if (tabs < 10) { *code_out = PALACE_SAM_EFIELDS; return; }
    if (tabs == 10 && lane == 0) L->c[11] = e + 1;
    __builtin_amdgcn_wave_barrier();
    int64_t c[12];
#pragma unroll
    for (int k = 0; k < 12; k++) c[k] = L->c[k];

    const SamHead h = sam_head(t, c, [&](const uint8_t *p, int64_t n) { return tid_of(names, p, n); });

    // the CIGAR, a byte per lane
    const int64_t ops_at = at + 36 + h.l_name, cb = c[5], ce = c[6] - 1;
    SamCigar cg{0, 0, 0, 0};
    if (!sam_is_star(t, cb, ce)) {
        bool bad = cb >= ce;
        for (int64_t p = cb; p < ce; p += kWave) {
            const int64_t q = p + lane;
            SamCigarByte x{false, false, 0, 0, 0};
            if (q < ce) x = sam_cigar_byte(t, cb, ce, q);
            const unsigned long long m = __ballot(x.op);
            if constexpr (kEncode) {
                const int64_t ord = cg.n_ops + __popcll(m & lanes_below(lane));
                if (x.op && ord < 65535) st32(o, ops_at + 4 * ord, x.word);
            }
            bad |= __ballot(x.bad) != 0;
            cg.n_ops += __popcll(m);
            cg.qlen += wave_sum(x.q);
            cg.rlen += wave_sum(x.r);
        }
        if (bad || cg.n_ops > 65535) cg.code = PALACE_SAM_ECIGAR;
    }

    // SEQ and QUAL
    const int64_t sb = c[9], se = c[10] - 1, qb = c[10], qe = c[11] - 1;
    const bool seq_star = sam_is_star(t, sb, se), qual_star = sam_is_star(t, qb, qe);
    const int64_t l_seq = seq_star ? 0 : se - sb;
    const int32_t seq_code = se == sb || l_seq > 0x7fffffffll ? PALACE_SAM_ESEQ : 0;
    const int32_t ciglen_code = cg.n_ops > 0 && !seq_star && cg.qlen != l_seq ? PALACE_SAM_ECIGLEN : 0;
    int32_t qual_code = 0;
    if (!qual_star) {
        if (qe - qb != l_seq || qe == qb) qual_code = PALACE_SAM_EQUAL;
        for (int64_t p = qb; p < qe && !qual_code; p += kWave) {
            const int64_t q = p + lane;
            if (__ballot(q < qe && !sam_qual_ok(t[q]))) qual_code = PALACE_SAM_EQUAL;
        }
    }
    const int64_t seq_at = ops_at + 4 * cg.n_ops, qual_at = seq_at + (l_seq + 1) / 2, aux_at = qual_at + l_seq;

    // the tags, kTagBatch at a time: their begins by ballot, a tag per lane, their places by a scan of their sizes
    int32_t tag_code = 0;
    int64_t aux = 0;
    for (int64_t p = c[11]; p <= e && !tag_code;) {
        if (lane == 0) L->tag[0] = p;
        int64_t n = 1;
        for (int64_t s = p; s < e && n <= kTagBatch; s += kWave) {
            const int64_t q = s + lane;
            const bool tab = q < e && t[q] == '\t';
            const unsigned long long m = __ballot(tab);
            if (tab) {
                const int64_t ord = n + __popcll(m & lanes_below(lane));
                if (ord <= kTagBatch) L->tag[ord] = q + 1;
            }
            n += __popcll(m);
        }
        const int nb = n <= kTagBatch ? static_cast<int>(n) : kTagBatch;
        if (n <= kTagBatch && lane == 0) L->tag[n] = e + 1;
        __builtin_amdgcn_wave_barrier();
        SamTag g{0, 0, 0, 0, 0};
        int64_t tb = 0, te = 0;
        if (lane < nb) {
            tb = L->tag[lane];
            te = L->tag[lane + 1] - 1;
            g = sam_tag(t, tb, te);
        }
        const int64_t next = L->tag[nb];
        __builtin_amdgcn_wave_barrier();                                     // (the next batch writes these words again)
        const unsigned long long bm = __ballot(g.code != 0);
        if (bm) { tag_code = __shfl(g.code, __ffsll(static_cast<long long>(bm)) - 1, 64); break; }
        if constexpr (kEncode) {
            const int64_t x = aux_at + aux + wave_exclusive(g.size, lane);
            if (lane < nb) sam_tag_write(t, tb, te, g, o, x);
            for (unsigned long long sm = __ballot(g.text > 0); sm; sm &= sm - 1) {       // the strings, by all lanes
                const int k = __ffsll(static_cast<long long>(sm)) - 1;
                const int64_t src = __shfl(static_cast<long long>(tb + 5), k, 64), len = __shfl(static_cast<long long>(g.text), k, 64),
                              dst = __shfl(static_cast<long long>(x + 3), k, 64);
                for (int64_t j = lane; j < len; j += kWave) o[dst + j] = t[src + j];
            }
        }
        aux += wave_sum(g.size);
        p = next;
    }

    *code_out = sam_first_code(h.code_a, cg.code, h.code_b, seq_code, ciglen_code, qual_code, tag_code);
    if (*code_out || (static_cast<uint32_t>(h.flag) & mask)) return;
    const int64_t size = 36 + h.l_name + 4 * cg.n_ops + (l_seq + 1) / 2 + l_seq + aux;
    *size_out = size;
    if constexpr (kEncode) {
        if (lane == 0) {
            sam_fixed_write(h, sam_fixed(h, cg), cg.n_ops, l_seq, size, o, at);
            o[at + 36 + h.l_name - 1] = 0;
        }
        for (int64_t k = lane; k < h.l_name - 1; k += kWave) o[at + 36 + k] = t[c[0] + k];
        for (int64_t j = lane; j < (l_seq + 1) / 2; j += kWave) o[seq_at + j] = static_cast<uint8_t>(sam_seq_byte(t, sb, l_seq, j));
        for (int64_t j = lane; j < l_seq; j += kWave) o[qual_at + j] = qual_star ? 0xff : static_cast<uint8_t>(t[qb + j] - 33);
    }
}

// size[i] = the record's bytes, 0 for a dropped line; *err = the smallest (line number << 8 | code)
__global__ __launch_bounds__(kSamThreads) void sam_plan_kernel(const uint8_t *t, const int64_t *start, int64_t n, int64_t line0, palace_bam_names names,
                                                               uint32_t mask, int32_t *size, unsigned long long *err)
{
    __shared__ WaveCuts cuts[kSamWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSamWaves + wave;
    if (i >= n) return;
    int32_t code = 0;
    int64_t sz = 0;
    sam_line_wave<false>(t, start[i], start[i + 1] - 1, names, mask, &cuts[wave], lane, &code, &sz, nullptr, 0);
    if (lane != 0) return;
    size[i] = static_cast<int32_t>(sz);
    if (code) atomicMin(err, static_cast<unsigned long long>(line0 + i) << 8 | static_cast<unsigned long long>(code));
}

// first launch of the two scans over the lines: bytes and kept lines in front, inside blocks of kScanThreads
__global__ __launch_bounds__(kScanThreads) void sam_scan_kernel(const int32_t *size, int64_t n, int64_t *off, int32_t *ord, long long *sum_bytes, long long *sum_kept)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    const long long v = i < n ? size[i] : 0;
    long long total_b, total_k;
    const long long ex_b = block_exclusive<long long, kScanThreads>(v, s_scan, &total_b);
    const long long ex_k = block_exclusive<long long, kScanThreads>(v ? 1 : 0, s_scan, &total_k);
    if (i < n) { off[i] = ex_b; ord[i] = static_cast<int32_t>(ex_k); }
    if (threadIdx.x == 0) { sum_bytes[blockIdx.x] = total_b; sum_kept[blockIdx.x] = total_k; }
}
__global__ __launch_bounds__(kScanThreads) void sam_base_kernel(int64_t n, int64_t head, int64_t *off, int32_t *ord, const long long *base_bytes,
                                                                const long long *base_kept, int64_t nb)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kScanThreads + threadIdx.x;
    if (i < n) {
        off[i] += base_bytes[blockIdx.x] + head;
        ord[i] += static_cast<int32_t>(base_kept[blockIdx.x]);
    }
    if (i == 0) off[n] = base_bytes[nb] + head;
}

__global__ __launch_bounds__(kSamThreads) void sam_encode_kernel(const uint8_t *t, const int64_t *start, int64_t n, palace_bam_names names, const int32_t *size,
                                                                 const int64_t *off, const int32_t *ord, uint8_t *out, int64_t *rec_start)
{
    __shared__ WaveCuts cuts[kSamWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSamWaves + wave;
    if (i >= n || size[i] == 0) return;
    int32_t code = 0;
    int64_t sz = 0;
    sam_line_wave<true>(t, start[i], start[i + 1] - 1, names, 0, &cuts[wave], lane, &code, &sz, out, off[i]);
    if (lane == 0) rec_start[ord[i]] = off[i] + 4;
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_sam_scratch_bytes(int64_t n)
{
    const int64_t nt = n > 0 ? (n + kLineTile - 1) / kLineTile : 0;
    return align256(static_cast<size_t>(nt + 1) * sizeof(long long));
}

extern "C" int palace_sam_lines(palace_ctx *ctx, const uint8_t *d_text, int64_t n, void *d_scratch, size_t scratch_bytes, int64_t *d_line_start, int64_t cap,
                                int64_t *out)
{
    PALACE_REQUIRE(ctx && n >= 0 && cap >= 0 && out, "bad argument");
    out[0] = 0;
    out[1] = out[2] = out[3] = out[4] = -1;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    if (n == 0) {
        if (d_line_start && cap >= 1) {
            PALACE_HIP_TRY(hipMemsetAsync(d_line_start, 0, sizeof(int64_t), ctx->stream));
            PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
            out[1] = out[2] = out[3] = out[4] = 0;
        }
        return PALACE_OK;
    }
    PALACE_REQUIRE(d_text && d_scratch, "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15) == 0, "the text must be 16-byte aligned");
    PALACE_REQUIRE(scratch_bytes >= palace_sam_scratch_bytes(n), "scratch smaller than palace_sam_scratch_bytes(n)");
    const int64_t nt = (n + kLineTile - 1) / kLineTile;
    PALACE_REQUIRE(nt < (1ll << 31), "text too long");
    long long *tiles = static_cast<long long *>(d_scratch), total = 0;
    hipLaunchKernelGGL(sam_count_kernel, dim3(static_cast<unsigned>(nt)), dim3(kLineThreads), 0, ctx->stream, d_text, n, tiles);
    hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, tiles, nt);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(&total, tiles + nt, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const int64_t n_lines = total + 1;
    out[0] = n_lines;
    if (!d_line_start || cap < n_lines + 1) return PALACE_OK;
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small);
    const unsigned long long init[3] = {~0ull, ~0ull, 0};
    unsigned long long got[3];
    PALACE_HIP_TRY(hipMemcpyAsync(small, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (init is this call's own)
    const int64_t nlb = (n_lines + 255) / 256;
    PALACE_REQUIRE(nlb < (1ll << 31), "too many lines");
    hipLaunchKernelGGL(sam_scatter_kernel, dim3(static_cast<unsigned>(nt)), dim3(kLineThreads), 0, ctx->stream, d_text, n, tiles, n_lines, d_line_start);
    hipLaunchKernelGGL(sam_first_kernel, dim3(static_cast<unsigned>(nlb)), dim3(256), 0, ctx->stream, d_text, d_line_start, n_lines, small);
    hipLaunchKernelGGL(sam_lines_err_kernel, dim3(static_cast<unsigned>(nlb)), dim3(256), 0, ctx->stream, d_text, d_line_start, n_lines, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(got, small, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    PALACE_REQUIRE(!got[2], "a line of more than 2^29 bytes");
    const int64_t n_header = got[0] == ~0ull ? n_lines : static_cast<int64_t>(got[0]);
    out[1] = n_header;
    out[2] = n_lines - n_header;
    out[3] = got[1] == ~0ull ? 0 : static_cast<int64_t>(got[1] >> 8);
    out[4] = got[1] == ~0ull ? 0 : static_cast<int64_t>(got[1] & 0xff);
    return PALACE_OK;
}

extern "C" int palace_sam_plan(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, int64_t line0, const palace_bam_names *names,
                               uint32_t mask, int64_t head_bytes, int32_t *d_size, int64_t *d_off, int32_t *d_ord, int64_t *out)
{
    PALACE_REQUIRE(ctx && n_lines >= 0 && line0 >= 1 && names && head_bytes >= 0 && d_off && out, "bad argument");
    PALACE_REQUIRE(n_lines < (1ll << 31), "more than 2^31 - 1 records");
    PALACE_REQUIRE(n_lines == 0 || (d_text && d_line_start && d_size && d_ord), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nb = (n_lines + kScanThreads - 1) / kScanThreads;
    const int rc = ensure_workspace(ctx, 2 * static_cast<size_t>(nb + 1) * sizeof(long long));
    if (rc) return rc;
    long long *sum_bytes = static_cast<long long *>(ctx->ws.ptr), *sum_kept = sum_bytes + nb + 1, got[2] = {0, 0};
    unsigned long long *err = reinterpret_cast<unsigned long long *>(ctx->d_small), e = ~0ull;
    PALACE_HIP_TRY(hipMemcpyAsync(err, &e, sizeof e, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (e is this call's own)
    if (nb == 0) PALACE_HIP_TRY(hipMemsetAsync(sum_bytes, 0, 2 * sizeof(long long), ctx->stream));
    else {
        hipLaunchKernelGGL(sam_plan_kernel, dim3(static_cast<unsigned>((n_lines + kSamWaves - 1) / kSamWaves)), dim3(kSamThreads), 0, ctx->stream, d_text,
                           d_line_start, n_lines, line0, *names, mask, d_size, err);
        hipLaunchKernelGGL(sam_scan_kernel, dim3(static_cast<unsigned>(nb)), dim3(kScanThreads), 0, ctx->stream, d_size, n_lines, d_off, d_ord, sum_bytes, sum_kept);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sum_bytes, nb);
        hipLaunchKernelGGL(block_sums_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sum_kept, nb);
    }
    hipLaunchKernelGGL(sam_base_kernel, dim3(static_cast<unsigned>(nb ? nb : 1)), dim3(kScanThreads), 0, ctx->stream, n_lines, head_bytes, d_off, d_ord, sum_bytes,
                       sum_kept, nb);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(&got[0], sum_bytes + nb, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(&got[1], sum_kept + nb, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(&e, err, sizeof e, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out[0] = got[1];
    out[1] = n_lines - got[1];
    out[2] = head_bytes + got[0];
    out[3] = e == ~0ull ? 0 : static_cast<int64_t>(e >> 8);
    out[4] = e == ~0ull ? 0 : static_cast<int64_t>(e & 0xff);
    return PALACE_OK;
}

extern "C" int palace_sam_encode(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, const palace_bam_names *names,
                                 const int32_t *d_size, const int64_t *d_off, const int32_t *d_ord, uint8_t *d_out, int64_t *d_starts)
{
    PALACE_REQUIRE(ctx && n_lines >= 0 && n_lines < (1ll << 31) && names, "bad argument");
    if (n_lines == 0) return PALACE_OK;
    PALACE_REQUIRE(d_text && d_line_start && d_size && d_off && d_ord && d_out && d_starts, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(sam_encode_kernel, dim3(static_cast<unsigned>((n_lines + kSamWaves - 1) / kSamWaves)), dim3(kSamThreads), 0, ctx->stream, d_text,
                       d_line_start, n_lines, *names, d_size, d_off, d_ord, d_out, d_starts);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
