// Paths -> FASTA on the device (include/palace_hip.h: palace_fasta_index .. palace_path_fasta_write): what the reference's
// make_fa_from_path.py does through pysam, as an index of the assembly's text, a hash table of its names and a gather.
//
// The index is four launches over tiles of 4096 bytes (256 lanes x 16, text_lanes.hpp), count -> scan -> records -> lines:
//   1. count: a tile's line ends (its LFs, and the text's end when the last line has no LF) and header starts ('>' at a line start);
//   2. scan: one workgroup gives every tile the lines and headers in front of it, the last line end before it and the first one
//      behind it -- with those a lane knows where the line of any of its line ends begins and where the next line ends, however
//      many tiles either spans;
//   3. records: the lane that owns a header line's end writes the record: name, seq_off, and bases / width of the line behind it;
//   4. lines: the lane that owns a sequence line's end adds its bases to its record's length (combined in the wavefront) and judges
//      the line BEHIND it against the record's first line; every lane checks the bytes of its own 16.
// A line's verdict needs the line itself, its neighbour and its record's first line: no running state, so no tiling shows in it.
// Faults are kept as the minimum of (line << 3 | code).
//
// The writer is paths_writer.hpp's, with this tool's token sizes and policy (below).
#include "common.hpp"
#include "fasta_names.hpp"
#include "paths_writer.hpp"

#include <climits>

namespace palace {
namespace {

constexpr int64_t kNone = INT64_MAX;

static_assert(kTileBytes == PALACE_FASTA_TILE_BYTES, "the header states the tile");
static_assert(sizeof(palace_fasta_rec) == 48, "record layout");
static_assert(sizeof(palace_fasta_status) == 24, "status layout");

// per tile, by the count kernel.  first_le / last_le: 1 + offset in the tile of its first / last line end (0: none)
struct Tile { uint32_t nl, nh, first_le, last_le; };
// per tile, by the scan kernel: lines that end and headers that start in front of it, the last line end in front of it (-1: none),
// the first line end behind it (kNone: none)
struct TileBase { int64_t line0, rec0, prev_le, next_le; };
struct Head { unsigned long long key; int64_t n_records; int32_t skip, pad[11]; };

inline size_t tiles_of(int64_t n) { return n <= 0 ? 0 : static_cast<size_t>((n + 1 + kTileBytes - 1) / kTileBytes); }   // (the text's end is a place too)

__device__ __forceinline__ uint32_t eq_mask(const uint32_t w[4], int valid, uint32_t c)
{
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t x = w[q] ^ (c * 0x01010101u);
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

// a lane's 16 bytes: its line ends (bit k = byte k; the text's end counts when the last line has no LF) and its header starts
struct Lane { uint32_t w[4]; int valid; uint32_t lmask, hmask; };
__device__ __forceinline__ Lane lane_of(const uint8_t *text, int64_t n, int64_t at)
{
    Lane l;
    l.valid = load_lane(text, n, at, l.w);
    const uint32_t nl = newline_mask(l.w, l.valid);
    const bool line_start = at == 0 || (at <= n && text[at - 1] == '\n');
    l.hmask = eq_mask(l.w, l.valid, '>') & ((nl << 1) | (line_start ? 1u : 0u)) & 0xffffu;
    l.lmask = nl;
    if (at <= n && n < at + kLaneBytes && text[n - 1] != '\n') l.lmask |= 1u << (n - at);
    return l;
}

// per lane, the tile offset of the last line end in the lanes before it (-1: none) and of the first in the lanes behind it (INT_MAX)
struct Around { int prev, next; };
__device__ __forceinline__ Around block_around(uint32_t lmask, int *s_last, int *s_first)
{
    const int tid = threadIdx.x;
    s_last[tid] = lmask ? tid * kLaneBytes + (31 - __clz(lmask)) : -1;
    s_first[tid] = lmask ? tid * kLaneBytes + (__ffs(lmask) - 1) : INT_MAX;
    __syncthreads();
    for (int d = 1; d < kTileThreads; d <<= 1) {
        const int a = tid >= d ? s_last[tid - d] : -1, b = tid + d < kTileThreads ? s_first[tid + d] : INT_MAX;
        __syncthreads();
        if (a > s_last[tid]) s_last[tid] = a;
        if (b < s_first[tid]) s_first[tid] = b;
        __syncthreads();
    }
    const Around r{tid ? s_last[tid - 1] : -1, tid + 1 < kTileThreads ? s_first[tid + 1] : INT_MAX};
    __syncthreads();
    return r;
}

// what a lane knows about the lines around its line ends
struct Where {
    int64_t tile0, at;
    uint32_t lmask, hmask, excl;          // excl: line ends (low 16 bits) and header starts in the tile's lanes before this one
    Around ar;
    TileBase tb;
    __device__ __forceinline__ int64_t prev_end(int k) const         // the line end before the one at bit k (-1: none)
    {
        const uint32_t below = lmask & ((1u << k) - 1u);
        return below ? at + (31 - __clz(below)) : ar.prev >= 0 ? tile0 + ar.prev : tb.prev_le;
    }
    __device__ __forceinline__ int64_t next_end(int k) const         // ... and the one behind it (kNone: none)
    {
        const uint32_t above = lmask & ~((2u << k) - 1u);
        return above ? at + (__ffs(above) - 1) : ar.next != INT_MAX ? tile0 + ar.next : tb.next_le;
    }
    __device__ __forceinline__ int64_t line_no(int k) const { return tb.line0 + (excl & 0xffffu) + __popc(lmask & ((1u << k) - 1u)) + 1; }   // 1-based
    __device__ __forceinline__ int64_t record(int k) const { return tb.rec0 + (excl >> 16) + __popc(hmask & ((2u << k) - 1u)) - 1; }       // -1: none yet
};

// bases and width of the line text[s .. e) whose end e is an LF (real) or the text's end
__device__ __forceinline__ void line_shape(const uint8_t *text, int64_t s, int64_t e, bool real, int64_t *bases, int64_t *width)
{
    *width = e - s + (real ? 1 : 0);
    *bases = e - s - ((real && e > s && text[e - 1] == '\r') ? 1 : 0);
}

__device__ __forceinline__ void fault(Head *head, int64_t line, int code)
{
    atomicMin(&head->key, (static_cast<unsigned long long>(line) << 3) | static_cast<unsigned>(code));
}

__global__ __launch_bounds__(kTileThreads) void fasta_count_kernel(const uint8_t *text, int64_t n, Tile *tiles)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    __shared__ uint32_t s_first, s_last;
    if (threadIdx.x == 0) { s_first = ~0u; s_last = 0; }
    const Lane l = lane_of(text, n, static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes);
    uint32_t total;
    block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(l.lmask)) | (static_cast<uint32_t>(__popc(l.hmask)) << 16), s_scan, &total);
    if (l.lmask) {
        atomicMin(&s_first, threadIdx.x * kLaneBytes + static_cast<uint32_t>(__ffs(l.lmask)));
        atomicMax(&s_last, threadIdx.x * kLaneBytes + static_cast<uint32_t>(32 - __clz(l.lmask)));
    }
    __syncthreads();
    if (threadIdx.x == 0) tiles[blockIdx.x] = Tile{total & 0xffffu, total >> 16, s_first == ~0u ? 0u : s_first, s_last};
}

__global__ __launch_bounds__(kScanThreads) void fasta_scan_kernel(const uint8_t *text, int64_t n, int64_t n_tiles, int64_t recs_cap, const Tile *tiles,
                                                                  TileBase *bases, Head *head)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    __shared__ long long s_first[kScanThreads], s_last[kScanThreads];
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t t0 = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    long long nl = 0, nh = 0, first = kNone, last = -1;
    for (int64_t k = t0; k < t1; k++) {
        const Tile t = tiles[k];
        nl += t.nl; nh += t.nh;
        if (t.nl) {
            if (first == kNone) first = k * kTileBytes + t.first_le - 1;
            last = k * kTileBytes + t.last_le - 1;
        }
    }
    long long nl_total, nh_total;
    long long line = block_exclusive<long long, kScanThreads>(nl, s_scan, &nl_total);
    long long rec = block_exclusive<long long, kScanThreads>(nh, s_scan, &nh_total);
    s_first[threadIdx.x] = first; s_last[threadIdx.x] = last;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = -1;
        for (int j = 0; j < kScanThreads; j++) { const long long v = s_last[j]; s_last[j] = run; run = v > run ? v : run; }
        run = kNone;
        for (int j = kScanThreads - 1; j >= 0; j--) { const long long v = s_first[j]; s_first[j] = run; run = v < run ? v : run; }
        head->n_records = nh_total;
        head->skip = nh_total > recs_cap ? 1 : 0;
        head->key = (n > 0 && text[0] != '>') ? ((1ull << 3) | PALACE_FASTA_ETEXT) : ~0ull;
    }
    __syncthreads();
    long long prev = s_last[threadIdx.x], next = s_first[threadIdx.x];
    for (int64_t k = t0; k < t1; k++) {
        const Tile t = tiles[k];
        bases[k].line0 = line; bases[k].rec0 = rec; bases[k].prev_le = prev;
        line += t.nl; rec += t.nh;
        if (t.nl) prev = k * kTileBytes + t.last_le - 1;
    }
    for (int64_t k = t1 - 1; k >= t0; k--) {
        bases[k].next_le = next;
        if (tiles[k].nl) next = k * kTileBytes + tiles[k].first_le - 1;
    }
}

__device__ __forceinline__ Where where_of(const Lane &l, const TileBase *bases, uint32_t *s_scan, int *s_last, int *s_first)
{
    Where w;
    w.tile0 = static_cast<int64_t>(blockIdx.x) * kTileBytes;
    w.at = w.tile0 + threadIdx.x * kLaneBytes;
    w.lmask = l.lmask; w.hmask = l.hmask;
    uint32_t total;
    w.excl = block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(l.lmask)) | (static_cast<uint32_t>(__popc(l.hmask)) << 16), s_scan, &total);
    w.ar = block_around(l.lmask, s_last, s_first);
    w.tb = bases[blockIdx.x];
    return w;
}

__global__ __launch_bounds__(kTileThreads) void fasta_records_kernel(const uint8_t *text, int64_t n, const TileBase *bases, Head *head, palace_fasta_rec *recs)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    __shared__ int s_last[kTileThreads], s_first[kTileThreads];
    if (head->skip) return;                                                  // (uniform)
    const Lane l = lane_of(text, n, static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes);
    const Where w = where_of(l, bases, s_scan, s_last, s_first);
    for (uint32_t m = l.lmask; m; m &= m - 1) {
        const int k = __ffs(m) - 1;
        const int64_t e = w.at + k, s = w.prev_end(k) + 1;
        if (text[s] != '>') continue;
        const bool real = e < n;
        int64_t j = s + 1;
        while (j < e && text[j] != ' ' && text[j] != '\t' && text[j] != '\r') j++;
        if (j == s + 1) fault(head, w.line_no(k), PALACE_FASTA_ENAME);
        palace_fasta_rec r{s + 1, j - (s + 1), real ? e + 1 : n, 0, 0, 0};
        if (real && e + 1 < n && text[e + 1] != '>') {                       // a line of this record follows: the first one
            const int64_t e2 = w.next_end(k);
            line_shape(text, e + 1, e2, e2 < n, &r.line_bases, &r.line_width);
        }
        recs[w.record(k)] = r;
    }
}

__global__ __launch_bounds__(kTileThreads) void fasta_lines_kernel(const uint8_t *text, int64_t n, const TileBase *bases, Head *head, palace_fasta_rec *recs)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    __shared__ int s_last[kTileThreads], s_first[kTileThreads];
    if (head->skip) return;                                                  // (uniform)
    const Lane l = lane_of(text, n, static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes);
    const Where w = where_of(l, bases, s_scan, s_last, s_first);
    // the lane's own bytes: those of sequence lines are 0x21-0x7E, LF, or a CR directly before an LF
    {
        const int64_t start = (w.ar.prev >= 0 ? w.tile0 + w.ar.prev : w.tb.prev_le) + 1;
        bool is_hdr = start < n && text[start] == '>';
        int64_t line = w.tb.line0 + (w.excl & 0xffffu) + 1;
#pragma unroll
        for (int k = 0; k < kLaneBytes; k++) {
            if (k >= l.valid) break;
            const uint32_t c = byte_of(l.w, k);
            const int64_t nxt = w.at + k + 1;
            if (c == '\n') { line++; is_hdr = nxt < n && text[nxt] == '>'; continue; }
            if (is_hdr || (c >= 0x21 && c <= 0x7e)) continue;
            if (c == '\r' && nxt < n && text[nxt] == '\n') continue;
            fault(head, line, PALACE_FASTA_EBYTE);
        }
    }
    // the lane's sequence lines: their bases, and the verdict on the line behind each
    long long cur = kNone;
    unsigned long long acc = 0;
    for (uint32_t m = l.lmask; m; m &= m - 1) {
        const int k = __ffs(m) - 1;
        const int64_t e = w.at + k, s = w.prev_end(k) + 1;
        if (text[s] == '>') continue;
        const int64_t r = w.record(k);
        if (r < 0) continue;                                                 // (text before the first header: ETEXT already)
        const bool real = e < n;
        int64_t b_p, w_p;
        line_shape(text, s, e, real, &b_p, &w_p);
        if (r != cur) {
            if (cur != kNone && acc) atomicAdd(reinterpret_cast<unsigned long long *>(&recs[cur].length), acc);
            cur = r; acc = 0;
        }
        acc += static_cast<unsigned long long>(b_p);
        if (!real || e + 1 >= n || text[e + 1] == '>') continue;
        const int64_t e2 = w.next_end(k);
        int64_t b_l, w_l;
        line_shape(text, e + 1, e2, e2 < n, &b_l, &w_l);
        if (b_l == 0) continue;
        const int64_t first_b = recs[r].line_bases, first_w = recs[r].line_width;
        const int code = b_p == 0 ? PALACE_FASTA_EBLANK : (b_p != first_b || w_p != first_w || b_l > first_b) ? PALACE_FASTA_ERAGGED : 0;
        if (code) fault(head, w.line_no(k) + 1, code);
    }
    // one atomic per wavefront for the record most of its lanes are in
    long long wave_r = cur;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(wave_r, d, 64);
        wave_r = wave_r < o ? wave_r : o;
    }
    unsigned long long mine = (cur == wave_r && cur != kNone) ? acc : 0;
    if (cur != wave_r && cur != kNone && acc) atomicAdd(reinterpret_cast<unsigned long long *>(&recs[cur].length), acc);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if ((threadIdx.x & 63) == 0 && wave_r != kNone && mine) atomicAdd(reinterpret_cast<unsigned long long *>(&recs[wave_r].length), mine);
}

// ---- the names ------------------------------------------------------------------------------------------------------------------

// linear probing without removals, as the BAM header's table (bam.hip) -- but the smallest record of a name stays
__global__ __launch_bounds__(256) void fasta_names_build_kernel(palace_fasta_names t)
{
    const int32_t r = static_cast<int32_t>(blockIdx.x * 256 + threadIdx.x);
    if (r >= t.n) return;
    const uint8_t *p = t.text + t.recs[r].name_off;
    const int64_t n = t.recs[r].name_len;
    for (uint32_t at = hash_name(p, n) & t.mask;; at = (at + 1) & t.mask) {
        const int32_t old = atomicCAS(&t.slots[at], -1, r);
        if (old < 0) return;
        if (is_name(t, old, p, n)) { atomicMin(&t.slots[at], r); return; }
    }
}

__global__ __launch_bounds__(256) void fasta_names_dup_kernel(palace_fasta_names t, uint8_t *dup)
{
    const int32_t r = static_cast<int32_t>(blockIdx.x * 256 + threadIdx.x);
    if (r >= t.n) return;
    dup[r] = record_of(t, t.text + t.recs[r].name_off, t.recs[r].name_len) != r ? 1 : 0;
}

__global__ __launch_bounds__(256) void path_resolve_kernel(palace_fasta_names t, const uint8_t *tok, const int64_t *off, int64_t n_tok, int32_t *code)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n_tok) return;
    const uint8_t *p = tok + off[i];
    const int64_t len = off[i + 1] - off[i];
    if (len <= 1) { code[i] = PALACE_PATH_NOTHING; return; }
    const uint8_t last = p[len - 1];
    const int64_t name_len = (last == '+' || last == '-') ? len - 1 : len;
    int32_t r = record_of(t, p, name_len), second = 0;
    if (r < 0) {
        int64_t j = name_len;
        while (j > 0 && p[j - 1] != '_') j--;
        r = record_of(t, p, j - 1);                                          // (no '_': the empty name)
        second = PALACE_PATH_SECOND_TRY;
    }
    code[i] = r < 0 ? PALACE_PATH_NOT_FOUND : (r << 2) | second | (last == '-' ? PALACE_PATH_REVERSE : 0);
}

// ---- the tokens' sizes and the writer's policy (paths_writer.hpp) --------------------------------------------------------------------

// a token's bytes: its record's bases
struct PathTokSize {
    const palace_fasta_rec *recs;
    const int32_t *code;
    __device__ __forceinline__ long long operator()(int64_t t) const { return code[t] >= 0 ? recs[code[t] >> 2].length : 0; }
};

// the tokens' bases and nothing between them; every path has its header and its LF
struct PathsPolicy {
    using Comp = ComplementAcgt;
    static constexpr bool kSeparator = false, kSkipEmptyPaths = false;
};

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_fasta_index_scratch_bytes(int64_t n)
{
    const size_t t = tiles_of(n);
    return align256(sizeof(Head)) + align256(t * sizeof(Tile)) + align256(t * sizeof(TileBase));
}

extern "C" int palace_fasta_index(palace_ctx *ctx, const uint8_t *d_text, int64_t n, palace_fasta_rec *d_recs, int64_t recs_cap, void *d_scratch,
                                  size_t scratch_bytes, palace_fasta_status *status_out)
{
    PALACE_REQUIRE(ctx && n >= 0 && recs_cap >= 0 && status_out && d_scratch, "bad argument");
    PALACE_REQUIRE((d_text || n == 0) && (d_recs || recs_cap == 0), "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15) == 0, "the text must be 16-byte aligned");
    PALACE_REQUIRE(scratch_bytes >= palace_fasta_index_scratch_bytes(n), "scratch smaller than palace_fasta_index_scratch_bytes(n)");
    const size_t nt = tiles_of(n);
    PALACE_REQUIRE(nt < (1ull << 31), "text too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    uint8_t *s = static_cast<uint8_t *>(d_scratch);
    Head *head = reinterpret_cast<Head *>(s);
    Tile *tiles = reinterpret_cast<Tile *>(s + align256(sizeof(Head)));
    TileBase *tb = reinterpret_cast<TileBase *>(s + align256(sizeof(Head)) + align256(nt * sizeof(Tile)));
    const dim3 grid(static_cast<unsigned>(nt)), block(kTileThreads);
    if (nt) hipLaunchKernelGGL(fasta_count_kernel, grid, block, 0, ctx->stream, d_text, n, tiles);
    hipLaunchKernelGGL(fasta_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_text, n, static_cast<int64_t>(nt), recs_cap, tiles, tb, head);
    if (nt) {
        hipLaunchKernelGGL(fasta_records_kernel, grid, block, 0, ctx->stream, d_text, n, tb, head, d_recs);
        hipLaunchKernelGGL(fasta_lines_kernel, grid, block, 0, ctx->stream, d_text, n, tb, head, d_recs);
    }
    PALACE_HIP_TRY(hipGetLastError());
    Head h;
    PALACE_HIP_TRY(hipMemcpyAsync(&h, head, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const bool bad = h.key != ~0ull;
    *status_out = palace_fasta_status{h.n_records, bad ? static_cast<int64_t>(h.key >> 3) : 0, bad ? static_cast<int32_t>(h.key & 7) : 0, 0};
    return PALACE_OK;
}

extern "C" int palace_fasta_names_create(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, int64_t n_records, uint8_t *d_dup,
                                         palace_fasta_names **out)
{
    PALACE_REQUIRE(ctx && out && n_records >= 0 && n_records < (1ll << 29), "bad argument (at most 2^29 - 1 records)");
    PALACE_REQUIRE(n_records == 0 || (d_text && d_recs), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    uint32_t cap = 64;
    while (cap < 2u * static_cast<uint32_t>(n_records)) cap <<= 1;
    palace_fasta_names *t = new palace_fasta_names{d_text, d_recs, static_cast<int32_t>(n_records), cap - 1, nullptr};
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->slots), static_cast<size_t>(cap) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(t->slots, 0xff, static_cast<size_t>(cap) * sizeof(int32_t), ctx->stream);      // every slot -1
    if (e == hipSuccess && n_records) {
        const dim3 grid((static_cast<unsigned>(n_records) + 255) / 256);
        hipLaunchKernelGGL(fasta_names_build_kernel, grid, dim3(256), 0, ctx->stream, *t);
        if (d_dup) hipLaunchKernelGGL(fasta_names_dup_kernel, grid, dim3(256), 0, ctx->stream, *t, d_dup);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        set_error("palace_fasta_names_create: %s", hipGetErrorString(e));
        if (t->slots) (void)hipFree(t->slots);
        delete t;
        return e == hipErrorOutOfMemory ? PALACE_ENOMEM : PALACE_EHIP;
    }
    *out = t;
    return PALACE_OK;
}

extern "C" int palace_fasta_names_destroy(palace_ctx *ctx, palace_fasta_names *names)
{
    if (!names) return PALACE_OK;
    PALACE_REQUIRE(ctx, "bad argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (a look-up may still be running)
    PALACE_HIP_TRY(hipFree(names->slots));
    delete names;
    return PALACE_OK;
}

extern "C" int palace_path_resolve(palace_ctx *ctx, const palace_fasta_names *names, const uint8_t *d_tok, const int64_t *d_tok_off, int64_t n_tok,
                                   int32_t *d_code)
{
    PALACE_REQUIRE(ctx && names && n_tok >= 0 && n_tok < (1ll << 39), "bad argument");
    if (n_tok == 0) return PALACE_OK;
    PALACE_REQUIRE(d_tok_off && d_code, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(path_resolve_kernel, dim3(static_cast<unsigned>((n_tok + 255) / 256)), dim3(256), 0, ctx->stream, *names, d_tok, d_tok_off, n_tok, d_code);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_path_fasta_lengths(palace_ctx *ctx, const palace_fasta_rec *d_recs, const int32_t *d_code, int64_t n_tok, const int64_t *d_path_off,
                                         int64_t n_paths, int64_t *d_tok_cum, int64_t *d_path_len)
{
    PALACE_REQUIRE(ctx && n_tok >= 0 && n_paths >= 0 && n_tok < (1ll << 39) && n_paths < (1ll << 39), "bad argument");
    PALACE_REQUIRE(d_tok_cum && d_path_off && (d_path_len || n_paths == 0) && (n_tok == 0 || (d_recs && d_code)), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    return paths_lengths(ctx, PathTokSize{d_recs, d_code}, n_tok, d_path_off, n_paths, d_tok_cum, d_path_len);
}

extern "C" int palace_path_fasta_write(palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code,
                                       const int64_t *d_tok_cum, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr,
                                       const int64_t *d_hdr_off, const int64_t *d_path_out, int64_t lo, int64_t hi, uint8_t *d_out)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && lo >= 0 && lo <= hi, "bad argument");
    return paths_write<PathsPolicy>(__func__, ctx, d_text, d_recs, d_code, d_tok_cum, d_path_off, n_paths, d_hdr, d_hdr_off, d_path_out, 0, lo, hi, d_out);
}
