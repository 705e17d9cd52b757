// The text of `samtools depth` on the device (palace:541): one line `contig <TAB> 1-based position <TAB> depth`
// per covered position, contigs in header order -- the bytes host/depthgz.hpp writes line by line on one thread.
//
// All contigs lie end to end in one global coordinate (as in depth.hip).  create: the match segments add +1 / -1 to an int32
// difference array (cut at their contig's end like depth_mark_kernel), an inclusive scan turns it into depths in place, and per
// tile of kTile positions the bytes, lines and depth sum of the tile's text are recorded and scanned exclusively in 64 bits.  A
// position's line has name + 1 + digits(position) + 1 + digits(depth) + 1 bytes, none where the depth is 0: where any byte of
// the text lies follows from the tile table and a scan inside one tile.  Memory: 4 B per position + 24 B per tile.
// emit writes any byte range of the text (a line may straddle either end); windows answers, per range of positions, where its
// lines start and how many they are -- what the tabix index of the file needs per 16 kb window.
// Integer sums only: the text does not depend on the order in which the segments arrive.
#include <algorithm>

#include "common.hpp"

namespace palace {
namespace {

constexpr int kTile = 1024, kTileThreads = 256, kPer = kTile / kTileThreads;

struct TileRec { uint64_t bytes, lines, sum; };                            // exclusive prefixes over the tiles; entry n_tiles = the totals

}  // namespace
}  // namespace palace

struct palace_depth_text {
    int32_t n_targets = 0;
    int64_t total_len = 0, n_tiles = 0;
    const int32_t *d_tlen = nullptr;                                        // the caller's
    const int64_t *d_tbase = nullptr, *d_name_off = nullptr;
    const uint8_t *d_names = nullptr;
    int32_t *d_depth = nullptr;                                             // total_len + 1
    palace::TileRec *d_tiles = nullptr;                                     // n_tiles + 1
    uint64_t text_bytes = 0, lines = 0, sum = 0;
};

namespace palace {
namespace {

__device__ __forceinline__ int digits_of(uint32_t v)
{
    return v < 10 ? 1 : v < 100 ? 2 : v < 1000 ? 3 : v < 10000 ? 4 : v < 100000 ? 5 : v < 1000000 ? 6 : v < 10000000 ? 7 : v < 100000000 ? 8
           : v < 1000000000 ? 9 : 10;
}

// the contig of global position g (0 <= g < total_len): the last one that starts at or before g (empty contigs in front of it start
// there too).  tbase has n_targets + 1 entries.
__device__ __forceinline__ int32_t contig_of(const int64_t *__restrict__ tbase, int32_t n_targets, int64_t g)
{
    int32_t lo = 0, hi = n_targets;                                        // first t with tbase[t] > g, in (lo, hi]
    while (lo < hi) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (tbase[mid] <= g) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

struct Names {
    const int64_t *tbase, *name_off;
    const uint8_t *names;
    int32_t n_targets;
};

// where a thread stands in the contigs: its positions mostly ascend, and stay in one contig for long
struct ContigCursor {
    int32_t t = -1;
    int64_t beg = 0, end = -1;
    int32_t name_len = 0;
    __device__ __forceinline__ void seek(const Names &nm, int64_t g)
    {
        if (t >= 0 && g >= beg && g < end) return;
        t = contig_of(nm.tbase, nm.n_targets, g);
        beg = nm.tbase[t]; end = nm.tbase[t + 1];
        name_len = static_cast<int32_t>(nm.name_off[t + 1] - nm.name_off[t]);
    }
    __device__ __forceinline__ uint32_t line_len(int64_t g, int32_t depth) const
    {
        return depth > 0 ? static_cast<uint32_t>(name_len + 3 + digits_of(static_cast<uint32_t>(g - beg + 1)) + digits_of(static_cast<uint32_t>(depth))) : 0u;
    }
};

// inclusive scan over a workgroup of kTileThreads; `total` = the workgroup's sum
template <class T>
__device__ __forceinline__ T block_scan(T v, T *wave_sum, T &total)
{
    const int tid = threadIdx.x;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if ((tid & 63) >= d) x += y;
    }
    __syncthreads();                                                       // (wave_sum may still be read from the call before)
    if ((tid & 63) == 63) wave_sum[tid >> 6] = x;
    __syncthreads();
    T before = 0, all = 0;
    for (int w = 0; w < kTileThreads / 64; w++) {
        if (w < (tid >> 6)) before += wave_sum[w];
        all += wave_sum[w];
    }
    total = all;
    return before + x;
}

__global__ __launch_bounds__(256) void dt_scatter_kernel(const int32_t *__restrict__ seg_tid, const int32_t *__restrict__ seg_pos,
                                                         const int32_t *__restrict__ seg_len, int64_t n, int32_t n_targets,
                                                         const int32_t *__restrict__ tlen, const int64_t *__restrict__ tbase,
                                                         int32_t *__restrict__ diff)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t t = seg_tid[i];
    const int64_t a = seg_pos[i], len = seg_len[i];
    if (t < 0 || t >= n_targets || a < 0 || len <= 0) return;
    const int64_t b = min(a + len, static_cast<int64_t>(tlen[t]));         // (a record that runs past its contig is cut there)
    if (b <= a) return;
    atomicAdd(&diff[tbase[t] + a], 1);
    atomicAdd(&diff[tbase[t] + b], -1);
}

// sum of the tile's differences -> tiles[tile].sum (as int64)
__global__ __launch_bounds__(kTileThreads) void dt_tile_sum_kernel(const int32_t *__restrict__ diff, int64_t total_len, TileRec *__restrict__ tiles)
{
    __shared__ int64_t wave_sum[kTileThreads / 64];
    const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kTile + threadIdx.x * kPer;
    int64_t v = 0;
    for (int k = 0; k < kPer; k++) if (g0 + k < total_len) v += diff[g0 + k];
    int64_t total;
    block_scan<int64_t>(v, wave_sum, total);
    if (threadIdx.x == 0) tiles[blockIdx.x].sum = static_cast<uint64_t>(total);
}

// exclusive scan of the three fields over all tiles (one workgroup); entry n_tiles = the totals
__global__ __launch_bounds__(kTileThreads) void dt_tile_scan_kernel(TileRec *__restrict__ tiles, int64_t n_tiles, int only_sum)
{
    __shared__ uint64_t wave_sum[kTileThreads / 64];
    uint64_t carry_b = 0, carry_l = 0, carry_s = 0;
    for (int64_t base = 0; base < n_tiles; base += kTileThreads) {
        const int64_t i = base + threadIdx.x;
        const TileRec r = i < n_tiles ? tiles[i] : TileRec{0, 0, 0};
        uint64_t tot;
        const uint64_t s = block_scan<uint64_t>(r.sum, wave_sum, tot);
        TileRec o{0, 0, carry_s + s - r.sum};
        carry_s += tot;
        if (!only_sum) {
            const uint64_t b = block_scan<uint64_t>(r.bytes, wave_sum, tot);
            o.bytes = carry_b + b - r.bytes; carry_b += tot;
            const uint64_t l = block_scan<uint64_t>(r.lines, wave_sum, tot);
            o.lines = carry_l + l - r.lines; carry_l += tot;
        }
        if (i < n_tiles) tiles[i] = o;
    }
    if (threadIdx.x == 0) tiles[n_tiles] = TileRec{carry_b, carry_l, carry_s};
}

// differences -> depths in place (tiles[tile].sum = the depth in front of the tile); the tile's bytes, lines and depth sum
__global__ __launch_bounds__(kTileThreads) void dt_depth_kernel(int32_t *__restrict__ depth, int64_t total_len, Names nm, TileRec *__restrict__ tiles)
{
    __shared__ int64_t wave_sum[kTileThreads / 64];
    __shared__ uint64_t wave_sum_u[kTileThreads / 64];
    const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kTile + threadIdx.x * kPer;
    int32_t d[kPer];
    int64_t v = 0;
    for (int k = 0; k < kPer; k++) { d[k] = g0 + k < total_len ? depth[g0 + k] : 0; v += d[k]; }
    int64_t total;
    const int64_t incl = block_scan<int64_t>(v, wave_sum, total);
    int64_t run = static_cast<int64_t>(tiles[blockIdx.x].sum) + incl - v;
    uint64_t bytes = 0, lines = 0, sum = 0;
    ContigCursor c;
    for (int k = 0; k < kPer; k++) {
        const int64_t g = g0 + k;
        if (g >= total_len) break;
        run += d[k];
        const int32_t dep = static_cast<int32_t>(run);
        depth[g] = dep;
        if (dep > 0) {
            c.seek(nm, g);
            bytes += c.line_len(g, dep); lines++; sum += static_cast<uint64_t>(dep);
        }
    }
    uint64_t tb, tl, ts;
    block_scan<uint64_t>(bytes, wave_sum_u, tb);
    block_scan<uint64_t>(lines, wave_sum_u, tl);
    block_scan<uint64_t>(sum, wave_sum_u, ts);
    __syncthreads();                                                       // (every thread has read tiles[tile].sum)
    if (threadIdx.x == 0) tiles[blockIdx.x] = TileRec{tb, tl, ts};
}

// first tile whose text ends behind byte `at` (tiles[i + 1].bytes > at); n_tiles if none
__device__ __forceinline__ int64_t tile_of_byte(const TileRec *__restrict__ tiles, int64_t n_tiles, uint64_t at)
{
    int64_t lo = 0, hi = n_tiles;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tiles[mid + 1].bytes > at) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// bytes [begin, end) of the text to out[0 ..): the workgroups share the tiles that hold them
__global__ __launch_bounds__(kTileThreads) void dt_emit_kernel(const int32_t *__restrict__ depth, int64_t total_len, Names nm,
                                                               const TileRec *__restrict__ tiles, int64_t n_tiles, uint64_t begin, uint64_t end,
                                                               uint8_t *__restrict__ out)
{
    __shared__ uint64_t wave_sum[kTileThreads / 64];
    const int64_t t_lo = tile_of_byte(tiles, n_tiles, begin), t_hi = tile_of_byte(tiles, n_tiles, end - 1);     // inclusive; < n_tiles as end <= all bytes
    for (int64_t tile = t_lo + blockIdx.x; tile <= t_hi && tile < n_tiles; tile += gridDim.x) {
        const uint64_t tile_at = tiles[tile].bytes;
        if (tiles[tile + 1].bytes == tile_at) continue;                    // (uniform)
        const int64_t g0 = tile * kTile + threadIdx.x * kPer;
        int32_t d[kPer];
        uint32_t ll[kPer];
        uint64_t mine = 0;
        ContigCursor c;
        for (int k = 0; k < kPer; k++) {
            const int64_t g = g0 + k;
            d[k] = g < total_len ? depth[g] : 0;
            ll[k] = 0;
            if (d[k] > 0) { c.seek(nm, g); ll[k] = c.line_len(g, d[k]); }
            mine += ll[k];
        }
        uint64_t tot;
        uint64_t at = tile_at + block_scan<uint64_t>(mine, wave_sum, tot) - mine;
        for (int k = 0; k < kPer; k++) {
            if (!ll[k]) continue;
            const int64_t g = g0 + k;
            const uint64_t l0 = at, l1 = at + ll[k];
            at = l1;
            if (l1 <= begin || l0 >= end) continue;
            c.seek(nm, g);
            char num[24];                                                  // "<TAB>position<TAB>depth<LF>", digits from the back
            int q = 24;
            num[--q] = '\n';
            for (uint32_t v = static_cast<uint32_t>(d[k]);; v /= 10) { num[--q] = static_cast<char>('0' + v % 10); if (v < 10) break; }
            num[--q] = '\t';
            for (uint32_t v = static_cast<uint32_t>(g - c.beg + 1);; v /= 10) { num[--q] = static_cast<char>('0' + v % 10); if (v < 10) break; }
            num[--q] = '\t';
            const uint8_t *name = nm.names + nm.name_off[c.t];
            const uint32_t nl = static_cast<uint32_t>(c.name_len);
            for (uint32_t j = 0; j < ll[k]; j++) {
                const uint64_t o = l0 + j;
                if (o >= begin && o < end) out[o - begin] = j < nl ? name[j] : static_cast<uint8_t>(num[q + static_cast<int>(j - nl)]);
            }
        }
    }
}

// text offset of the first line at or behind global position g, and the lines in front of it: one wavefront per query
__device__ __forceinline__ void prefix_at(const int32_t *__restrict__ depth, int64_t total_len, const Names &nm, const TileRec *__restrict__ tiles,
                                          int64_t n_tiles, int64_t g, uint64_t &bytes, uint64_t &lines)
{
    const int lane = threadIdx.x & 63;
    if (g >= total_len) { bytes = tiles[n_tiles].bytes; lines = tiles[n_tiles].lines; return; }
    const int64_t tile = g / kTile;
    uint64_t b = 0, l = 0;
    ContigCursor c;
    for (int64_t p = tile * kTile + lane; p < g; p += 64) {
        const int32_t dep = depth[p];
        if (dep > 0) { c.seek(nm, p); b += c.line_len(p, dep); l++; }
    }
    for (int d = 32; d; d >>= 1) { b += __shfl_xor(b, d, 64); l += __shfl_xor(l, d, 64); }
    bytes = tiles[tile].bytes + b; lines = tiles[tile].lines + l;
}

__global__ __launch_bounds__(256) void dt_windows_kernel(const int32_t *__restrict__ depth, int64_t total_len, Names nm,
                                                         const TileRec *__restrict__ tiles, int64_t n_tiles, int64_t n_windows,
                                                         const int64_t *__restrict__ win_beg, const int64_t *__restrict__ win_end,
                                                         uint64_t *__restrict__ text_beg, uint64_t *__restrict__ text_end, uint64_t *__restrict__ n_lines)
{
    const int64_t w = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (w >= n_windows) return;
    const int64_t g0 = max(static_cast<int64_t>(0), win_beg[w]), g1 = max(g0, win_end[w]);
    uint64_t b0, l0, b1, l1;
    prefix_at(depth, total_len, nm, tiles, n_tiles, g0, b0, l0);
    prefix_at(depth, total_len, nm, tiles, n_tiles, g1, b1, l1);
    if ((threadIdx.x & 63) == 0) { text_beg[w] = b0; text_end[w] = b1; n_lines[w] = l1 - l0; }
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_depth_text_destroy(palace_ctx *ctx, palace_depth_text *dt)
{
    if (!dt) return PALACE_OK;
    PALACE_REQUIRE(ctx, "bad argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (dt->d_depth) (void)hipFree(dt->d_depth);
    if (dt->d_tiles) (void)hipFree(dt->d_tiles);
    delete dt;
    return PALACE_OK;
}

extern "C" int palace_depth_text_create(palace_ctx *ctx, int64_t n_segs, const int32_t *d_seg_tid, const int32_t *d_seg_pos,
                                        const int32_t *d_seg_len, int32_t n_targets, const int32_t *d_tlen, const int64_t *d_tbase,
                                        int64_t total_len, const uint8_t *d_names, const int64_t *d_name_off, palace_depth_text **out,
                                        uint64_t *text_bytes_out, uint64_t *lines_out, uint64_t *sum_out)
{
    PALACE_REQUIRE(ctx && out && text_bytes_out && lines_out && sum_out && n_segs >= 0 && n_targets >= 0 && total_len >= 0, "bad argument");
    PALACE_REQUIRE(n_targets == 0 || (d_tlen && d_tbase && d_names && d_name_off), "null device pointer");
    PALACE_REQUIRE(n_segs == 0 || (d_seg_tid && d_seg_pos && d_seg_len), "null device pointer");
    PALACE_REQUIRE((n_segs + 255) / 256 < (1ll << 31) && (total_len + kTile - 1) / kTile < (1ll << 31), "too large for one launch");
    *out = nullptr; *text_bytes_out = 0; *lines_out = 0; *sum_out = 0;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    palace_depth_text *dt = new palace_depth_text;
    dt->n_targets = n_targets; dt->total_len = total_len; dt->n_tiles = (total_len + kTile - 1) / kTile;
    dt->d_tlen = d_tlen; dt->d_tbase = d_tbase; dt->d_names = d_names; dt->d_name_off = d_name_off;
    auto fail = [&](hipError_t e, const char *what) {
        set_error("%s failed: %s", what, hipGetErrorString(e));
        if (dt->d_depth) (void)hipFree(dt->d_depth);
        if (dt->d_tiles) (void)hipFree(dt->d_tiles);
        delete dt;
        return PALACE_EHIP;
    };
    hipError_t e;
    if ((e = hipMalloc(reinterpret_cast<void **>(&dt->d_depth), static_cast<size_t>(total_len + 1) * 4)) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMalloc(reinterpret_cast<void **>(&dt->d_tiles), static_cast<size_t>(dt->n_tiles + 1) * sizeof(TileRec))) != hipSuccess) return fail(e, "hipMalloc");
    if ((e = hipMemsetAsync(dt->d_depth, 0, static_cast<size_t>(total_len + 1) * 4, ctx->stream)) != hipSuccess) return fail(e, "hipMemsetAsync");
    const Names nm{d_tbase, d_name_off, d_names, n_targets};
    const unsigned nt = static_cast<unsigned>(dt->n_tiles);
    if (n_segs && n_targets)
        hipLaunchKernelGGL(dt_scatter_kernel, dim3(static_cast<unsigned>((n_segs + 255) / 256)), dim3(256), 0, ctx->stream, d_seg_tid, d_seg_pos,
                           d_seg_len, n_segs, n_targets, d_tlen, d_tbase, dt->d_depth);
    if (nt) hipLaunchKernelGGL(dt_tile_sum_kernel, dim3(nt), dim3(kTileThreads), 0, ctx->stream, dt->d_depth, total_len, dt->d_tiles);
    hipLaunchKernelGGL(dt_tile_scan_kernel, dim3(1), dim3(kTileThreads), 0, ctx->stream, dt->d_tiles, dt->n_tiles, 1);
    if (nt) hipLaunchKernelGGL(dt_depth_kernel, dim3(nt), dim3(kTileThreads), 0, ctx->stream, dt->d_depth, total_len, nm, dt->d_tiles);
    hipLaunchKernelGGL(dt_tile_scan_kernel, dim3(1), dim3(kTileThreads), 0, ctx->stream, dt->d_tiles, dt->n_tiles, 0);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "kernel launch");
    TileRec tot;
    if ((e = hipMemcpyAsync(&tot, dt->d_tiles + dt->n_tiles, sizeof tot, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return fail(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e, "hipStreamSynchronize");
    dt->text_bytes = tot.bytes; dt->lines = tot.lines; dt->sum = tot.sum;
    *text_bytes_out = tot.bytes; *lines_out = tot.lines; *sum_out = tot.sum;
    *out = dt;
    return PALACE_OK;
}

extern "C" int palace_depth_text_emit(palace_ctx *ctx, const palace_depth_text *dt, uint64_t text_begin, uint64_t text_end, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && dt && text_begin <= text_end && text_end <= dt->text_bytes, "bad argument");
    if (text_begin == text_end) return PALACE_OK;
    PALACE_REQUIRE(d_out, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const Names nm{dt->d_tbase, dt->d_name_off, dt->d_names, dt->n_targets};
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(dt->n_tiles, kCUs * 16));
    hipLaunchKernelGGL(dt_emit_kernel, dim3(grid), dim3(kTileThreads), 0, ctx->stream, dt->d_depth, dt->total_len, nm, dt->d_tiles, dt->n_tiles,
                       text_begin, text_end, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_depth_text_windows(palace_ctx *ctx, const palace_depth_text *dt, int64_t n_windows, const int64_t *d_win_beg,
                                         const int64_t *d_win_end, uint64_t *d_text_beg, uint64_t *d_text_end, uint64_t *d_lines)
{
    PALACE_REQUIRE(ctx && dt && n_windows >= 0 && (n_windows + 3) / 4 < (1ll << 31), "bad argument");
    if (n_windows == 0) return PALACE_OK;
    PALACE_REQUIRE(d_win_beg && d_win_end && d_text_beg && d_text_end && d_lines, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const Names nm{dt->d_tbase, dt->d_name_off, dt->d_names, dt->n_targets};
    hipLaunchKernelGGL(dt_windows_kernel, dim3(static_cast<unsigned>((n_windows + 3) / 4)), dim3(256), 0, ctx->stream, dt->d_depth, dt->total_len,
                       nm, dt->d_tiles, dt->n_tiles, n_windows, d_win_beg, d_win_end, d_text_beg, d_text_end, d_lines);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
