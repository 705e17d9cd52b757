// The inflated BAM stream in HBM -> where its alignment records start (palace_bam_walk) and the match segments of the depth stage
// (palace_bam_match_segments): what `bamdepth --bam-gpu` needs to take a BAM without its records crossing PCIe again
// (include/palace_hip.h; the host's statement of both is host/bam.cpp: BamLoad::walk_step and decode_range).
//
// The record walk is serial by format -- a record's size is its first word -- and its result is DEFINED as that serial walk from
// the first record.  What runs in parallel is a guess that is checked, never trusted:
//   1. guess: the stream behind the header is cut into chunks; one wavefront per chunk tests 64 consecutive offsets per step for
//      "a record could start here" (the walk's own rules, refID / next_refID in [-1, n_ref), pos and next_pos >= -1, the name's
//      last byte NUL, and the same for kSuccessors records behind it), a ballot takes the first survivor, and the wave walks its
//      chunk from there: records counted, the offset at which the walk leaves the chunk (or ends) noted.  Chunk 0 starts at the
//      first record, exactly.
//   2. chain: one wavefront visits the chunks in stream order from the first record.  A chunk the chain enters at its guess counts
//      as it is -- the walk from an offset depends on nothing but the bytes, so it IS the serial walk from there; a chunk entered
//      anywhere else is walked again from the true entry by the chain itself; a chunk the chain jumps over (a record longer than
//      a chunk) counts for nothing; the first failing step ends everything.  The chain hands every chunk its place in the output
//      as it goes: the scan of the counts costs nothing extra.
//   3. starts: one thread per chunk walks its counted records again and writes their starts.
// Whatever the bytes are, the result is the serial walk's; only the time depends on them (a stream built to defeat every guess
// is walked by the chain alone: one wave, one dependent load per record).  Every read lies inside [0, total): a step reads the
// four bytes of its size word only when they are there and a record's fields only when the whole record is.
#include "common.hpp"

namespace palace {
namespace {

constexpr int64_t kDefaultChunk = 65536, kMinChunk = 64;
constexpr int kSuccessors = 3;          // records behind a candidate that must look like records too

// per chunk: entry = the guess (-1: none), after the chain the offset the serial walk enters the chunk at; count = records that
// start in the chunk walking from entry; exit = where that walk leaves the chunk or ends; base = records in front of the chunk
struct ChunkRec { int64_t entry, exit, base; int32_t count, flags; };
constexpr int32_t kEnded = 1, kUsed = 2;
// [0] records, [1] stop offset, [2..5] chunks, guesses that held, chunks repaired, chunks without a start
struct WalkHead { int64_t v[8]; };

// unaligned-safe loads: the stream has no alignment anywhere
__device__ __forceinline__ uint32_t ld16(const uint8_t *d, int64_t p) { return d[p] | (static_cast<uint32_t>(d[p + 1]) << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t *d, int64_t p)
{
    return d[p] | (static_cast<uint32_t>(d[p + 1]) << 8) | (static_cast<uint32_t>(d[p + 2]) << 16) | (static_cast<uint32_t>(d[p + 3]) << 24);
}

// BamLoad::walk_step (host/bam.cpp) on a stream that is there in full: true = a record at p, *next = the offset behind it
__device__ __forceinline__ bool walk_step(const uint8_t *d, int64_t p, int64_t total, int64_t *next)
{
    if (p + 4 > total) return false;
    const int64_t bs = ld32(d, p);
    if (bs < 32) return false;
    if (p + 4 + bs > total) return false;
    const int64_t r = p + 4;
    const int64_t l_name = d[r + 8], n_cig = ld16(d, r + 12), l_seq = ld32(d, r + 16);
    if (l_name < 1 || l_seq > 0x7fffffffll || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) return false;
    *next = p + 4 + bs;
    return true;
}

// the guess's test: a step of the walk, and the fields a real record keeps in range
__device__ __forceinline__ bool looks_like_record(const uint8_t *d, int64_t p, int64_t total, int32_t n_ref, int64_t *next)
{
    if (!walk_step(d, p, total, next)) return false;
    const int64_t r = p + 4;
    const int32_t tid = static_cast<int32_t>(ld32(d, r)), pos = static_cast<int32_t>(ld32(d, r + 4));
    const int32_t mtid = static_cast<int32_t>(ld32(d, r + 20)), mpos = static_cast<int32_t>(ld32(d, r + 24));
    if (tid < -1 || tid >= n_ref || mtid < -1 || mtid >= n_ref || pos < -1 || mpos < -1) return false;
    return d[r + 32 + d[r + 8] - 1] == 0;
}

__device__ __forceinline__ bool candidate(const uint8_t *d, int64_t p, int64_t total, int32_t n_ref)
{
    int64_t q = p;
    for (int k = 0; k <= kSuccessors; k++) {
        if (k && q == total) return true;                                    // the stream ends behind a record: nothing more to ask
        if (!looks_like_record(d, q, total, n_ref, &q)) return false;
    }
    return true;
}

// the serial walk from `entry` while it is in front of chunk_end
__device__ __forceinline__ void walk_chunk(const uint8_t *d, int64_t total, int64_t entry, int64_t chunk_end, ChunkRec *r)
{
    int64_t p = entry;
    int32_t n = 0, flags = 0;
    while (p < chunk_end) {
        int64_t next;
        if (!walk_step(d, p, total, &next)) { flags = kEnded; break; }
        n++;
        p = next;
    }
    r->entry = entry; r->exit = p; r->count = n; r->flags = flags; r->base = 0;
}

__global__ __launch_bounds__(64) void bam_guess_kernel(const uint8_t *d, int64_t total, int64_t first, int32_t n_ref, int64_t chunk,
                                                       int64_t n_chunks, ChunkRec *tab)
{
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    if (c >= n_chunks) return;
    const int64_t lo = first + c * chunk, hi = lo + chunk < total ? lo + chunk : total;
    int64_t guess = c == 0 ? first : -1;
    if (c)
        for (int64_t b = lo; b < hi; b += 64) {                              // (uniform)
            const int64_t p = b + lane;
            const unsigned long long m = __ballot(p < hi && candidate(d, p, total, n_ref));
            if (m) { guess = b + (__ffsll(m) - 1); break; }
        }
    ChunkRec r{-1, 0, 0, 0, 0};
    if (guess >= 0) walk_chunk(d, total, guess, lo + chunk, &r);             // (every lane the same walk: the loads are broadcasts)
    if (lane == 0) tab[c] = r;
}

__global__ __launch_bounds__(64) void bam_chain_kernel(const uint8_t *d, int64_t total, int64_t first, int64_t chunk, int64_t n_chunks,
                                                       ChunkRec *tab, WalkHead *head)
{
    __shared__ ChunkRec win[64];                                             // the table around the chain's chunk: one load per 64 chunks
    const int lane = threadIdx.x;
    long long none = 0;
    for (int64_t c = lane; c < n_chunks; c += 64) none += tab[c].entry < 0;
    for (int s = 32; s >= 1; s >>= 1) none += __shfl_xor(none, s, 64);
    int64_t p = first, n = 0, held = 0, repaired = 0, stop = first, win_base = -64;
    for (;;) {                                                               // (uniform: every lane follows the same chain)
        const int64_t c = (p - first) / chunk;
        if (c >= n_chunks) { stop = p; break; }                              // p == total behind the last chunk
        if (c < win_base || c >= win_base + 64) {
            __syncthreads();
            if (c + lane < n_chunks) win[lane] = tab[c + lane];
            win_base = c;
            __syncthreads();
        }
        ChunkRec r = win[c - win_base];
        if (r.entry == p) held++;
        else { repaired++; walk_chunk(d, total, p, first + (c + 1) * chunk, &r); }
        r.base = n;
        r.flags |= kUsed;
        n += r.count;
        if (lane == 0) tab[c] = r;
        if (r.flags & kEnded) { stop = r.exit; break; }
        p = r.exit;
    }
    if (lane == 0) head[0] = WalkHead{{n, stop, n_chunks, held, repaired, static_cast<int64_t>(none), 0, 0}};
}

__global__ __launch_bounds__(256) void bam_starts_kernel(const uint8_t *d, int64_t n_chunks, const ChunkRec *tab, int64_t *starts, int64_t cap)
{
    const int64_t c = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (c >= n_chunks) return;
    const ChunkRec r = tab[c];
    if (!(r.flags & kUsed)) return;
    int64_t p = r.entry;
    for (int64_t k = r.base; k < r.base + r.count && k < cap; k++) {         // (counted records: each passed the walk's step)
        starts[k] = p + 4;
        p += 4 + static_cast<int64_t>(ld32(d, p));
    }
}

// ---- match segments: decode_range's mseg_* (host/bam.cpp) --------------------------------------------------------------------

// size of one aux value at v (type byte consumed); 0 = unknown type or malformed (aux_size of the host)
__device__ __forceinline__ uint64_t aux_size(const uint8_t *d, uint32_t type, int64_t v, int64_t end)
{
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H':
        for (int64_t q = v; q < end; q++)
            if (d[q] == 0) return static_cast<uint64_t>(q - v + 1);
        return 0;
    case 'B': {
        if (end - v < 5) return 0;
        uint64_t es;
        switch (d[v]) {
        case 'c': case 'C': es = 1; break;
        case 's': case 'S': es = 2; break;
        case 'i': case 'I': case 'f': es = 4; break;
        default: return 0;
        }
        return 5 + es * static_cast<uint64_t>(ld32(d, v + 1));
    }
    default: return 0;
    }
}

// f(tid, pos, len) for every match segment of the record whose refID lies at s, in operation order
template <class F>
__device__ __forceinline__ void record_segments(const uint8_t *d, int64_t s, int32_t n_ref, F f)
{
    const int64_t end = s + static_cast<int64_t>(ld32(d, s - 4));
    const int32_t tid = static_cast<int32_t>(ld32(d, s)), pos = static_cast<int32_t>(ld32(d, s + 4));
    const uint32_t flag = ld16(d, s + 14);
    if ((flag & 0x704u) || tid < 0 || tid >= n_ref || pos < 0) return;       // what `samtools depth` does not count
    const int64_t l_name = d[s + 8], n_cig = ld16(d, s + 12), l_seq = ld32(d, s + 16);
    const int64_t cg = s + 32 + l_name;
    int64_t ops = cg, n_ops = n_cig;
    // a CIGAR of more than 65535 ops: the CG:B,I tag behind the <l_seq>S<ref>N placeholder (SAM spec 4.2.2)
    if (n_cig > 0 && (ld32(d, cg) & 15u) == 4 && static_cast<int64_t>(ld32(d, cg) >> 4) == l_seq) {
        for (int64_t x = cg + 4 * n_cig + (l_seq + 1) / 2 + l_seq; x + 3 <= end;) {
            const int64_t v = x + 3;
            const uint32_t type = d[x + 2];
            const uint64_t sz = aux_size(d, type, v, end);
            if (!sz || sz > static_cast<uint64_t>(end - v)) break;
            if (d[x] == 'C' && d[x + 1] == 'G') {                            // the first CG tag decides
                if (type == 'B' && (d[v] == 'I' || d[v] == 'i') && ld32(d, v + 1) >= static_cast<uint32_t>(n_cig) && ld32(d, v + 1) < (1u << 29)) {
                    ops = v + 5;
                    n_ops = ld32(d, v + 1);
                }
                break;
            }
            x = v + static_cast<int64_t>(sz);
        }
    }
    uint32_t rl = 0;
    for (int64_t k = 0; k < n_ops; k++) {
        const uint32_t w = ld32(d, ops + 4 * k), op = w & 15u, len = w >> 4;
        if (len > 0 && (op == 0 || op == 7 || op == 8)) f(tid, static_cast<int32_t>(static_cast<uint32_t>(pos) + rl), static_cast<int32_t>(len));
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) rl += len;
    }
}

constexpr int kSegThreads = 256, kScanThreads = 1024;

template <class T, int nthreads>
__device__ __forceinline__ T block_exclusive(T v, T *lds, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T o = __shfl_up(inc, s, 64);
        if (lane >= s) inc += o;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        T run = 0;
        for (int k = 0; k < nthreads / 64; k++) { const T t = lds[k]; lds[k] = run; run += t; }
        lds[nthreads / 64] = run;
    }
    __syncthreads();
    const T out = lds[wave] + inc - v;
    *total = lds[nthreads / 64];
    __syncthreads();
    return out;
}

__device__ __forceinline__ long long segments_of(const uint8_t *d, const int64_t *starts, int64_t i, int64_t n, int32_t n_ref)
{
    long long cnt = 0;
    if (i < n) record_segments(d, starts[i], n_ref, [&](int32_t, int32_t, int32_t) { cnt++; });
    return cnt;
}

__global__ __launch_bounds__(kSegThreads) void bam_seg_count_kernel(const uint8_t *d, const int64_t *starts, int64_t n, int32_t n_ref,
                                                                    long long *block_sum)
{
    __shared__ long long lds[kSegThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSegThreads + threadIdx.x;
    long long total;
    block_exclusive<long long, kSegThreads>(segments_of(d, starts, i, n, n_ref), lds, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one workgroup: block_sum[b] becomes the segments in front of block b, block_sum[n_blocks] their total
__global__ __launch_bounds__(kScanThreads) void bam_seg_scan_kernel(long long *block_sum, int64_t n_blocks)
{
    __shared__ long long lds[kScanThreads / 64 + 1];
    const int64_t per = (n_blocks + kScanThreads - 1) / kScanThreads;
    const int64_t b0 = threadIdx.x * per < n_blocks ? threadIdx.x * per : n_blocks, b1 = b0 + per < n_blocks ? b0 + per : n_blocks;
    long long mine = 0, total;
    for (int64_t b = b0; b < b1; b++) mine += block_sum[b];
    long long run = block_exclusive<long long, kScanThreads>(mine, lds, &total);
    for (int64_t b = b0; b < b1; b++) { const long long t = block_sum[b]; block_sum[b] = run; run += t; }
    if (threadIdx.x == 0) block_sum[n_blocks] = total;
}

__global__ __launch_bounds__(kSegThreads) void bam_seg_emit_kernel(const uint8_t *d, const int64_t *starts, int64_t n, int32_t n_ref,
                                                                   const long long *block_base, int32_t *seg_tid, int32_t *seg_pos,
                                                                   int32_t *seg_len, int64_t cap)
{
    __shared__ long long lds[kSegThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSegThreads + threadIdx.x;
    long long total;
    long long at = block_base[blockIdx.x] + block_exclusive<long long, kSegThreads>(segments_of(d, starts, i, n, n_ref), lds, &total);
    if (i >= n) return;
    record_segments(d, starts[i], n_ref, [&](int32_t tid, int32_t pos, int32_t len) {
        if (at < cap) { seg_tid[at] = tid; seg_pos[at] = pos; seg_len[at] = len; }
        at++;
    });
}

inline int64_t chunk_bytes(int64_t chunk) { return chunk <= 0 ? kDefaultChunk : chunk < kMinChunk ? kMinChunk : chunk; }
inline int64_t chunks_of(int64_t total, int64_t first, int64_t chunk)
{
    const int64_t n = (total - first + chunk - 1) / chunk;
    return n > 0 ? n : 1;
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_bam_walk_scratch_bytes(int64_t total, int64_t first, int64_t chunk)
{
    if (total < 0 || first < 0 || first > total) return 0;
    return sizeof(WalkHead) + static_cast<size_t>(chunks_of(total, first, chunk_bytes(chunk))) * sizeof(ChunkRec);
}

extern "C" int palace_bam_walk_starts(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, int64_t first, int64_t chunk, const void *d_scratch,
                                      size_t scratch_bytes, int64_t *d_starts, int64_t cap)
{
    PALACE_REQUIRE(ctx && total >= 0 && first >= 0 && first <= total && cap >= 0, "bad argument");
    PALACE_REQUIRE(d_scratch && scratch_bytes >= palace_bam_walk_scratch_bytes(total, first, chunk), "scratch smaller than palace_bam_walk_scratch_bytes()");
    if (cap == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t nc = chunks_of(total, first, chunk_bytes(chunk));
    const ChunkRec *tab = reinterpret_cast<const ChunkRec *>(static_cast<const uint8_t *>(d_scratch) + sizeof(WalkHead));
    hipLaunchKernelGGL(bam_starts_kernel, dim3(static_cast<unsigned>((nc + 255) / 256)), dim3(256), 0, ctx->stream, d_stream, nc, tab, d_starts, cap);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bam_walk(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, int64_t first, int32_t n_ref, int64_t chunk,
                               void *d_scratch, size_t scratch_bytes, int64_t *d_starts, int64_t cap, int64_t *n_records_out,
                               int64_t *stop_out, int64_t stats_out[4])
{
    PALACE_REQUIRE(ctx && total >= 0 && first >= 0 && first <= total && cap >= 0 && n_records_out, "bad argument");
    PALACE_REQUIRE((d_stream || total == 0) && (d_starts || cap == 0), "null device pointer");
    PALACE_REQUIRE(d_scratch && scratch_bytes >= palace_bam_walk_scratch_bytes(total, first, chunk), "scratch smaller than palace_bam_walk_scratch_bytes()");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t cb = chunk_bytes(chunk), nc = chunks_of(total, first, cb);
    PALACE_REQUIRE(nc < (1ll << 31), "too many chunks: raise the chunk size");
    WalkHead *head = static_cast<WalkHead *>(d_scratch);
    ChunkRec *tab = reinterpret_cast<ChunkRec *>(static_cast<uint8_t *>(d_scratch) + sizeof(WalkHead));
    hipLaunchKernelGGL(bam_guess_kernel, dim3(static_cast<unsigned>(nc)), dim3(64), 0, ctx->stream, d_stream, total, first, n_ref, cb, nc, tab);
    hipLaunchKernelGGL(bam_chain_kernel, dim3(1), dim3(64), 0, ctx->stream, d_stream, total, first, cb, nc, tab, head);
    PALACE_HIP_TRY(hipGetLastError());
    WalkHead h;
    PALACE_HIP_TRY(hipMemcpyAsync(&h, head, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_records_out = h.v[0];
    if (stop_out) *stop_out = h.v[1];
    if (stats_out) for (int k = 0; k < 4; k++) stats_out[k] = h.v[2 + k];
    if (d_starts && h.v[0] <= cap) return palace_bam_walk_starts(ctx, d_stream, total, first, chunk, d_scratch, scratch_bytes, d_starts, cap);
    return PALACE_OK;
}

extern "C" int palace_bam_match_segments(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                                         int32_t n_ref, int32_t *d_seg_tid, int32_t *d_seg_pos, int32_t *d_seg_len, int64_t cap,
                                         int64_t *n_segs_out)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0 && cap >= 0 && n_segs_out, "bad argument");
    const bool emit = d_seg_tid || d_seg_pos || d_seg_len;
    PALACE_REQUIRE(!emit || (d_seg_tid && d_seg_pos && d_seg_len), "give all three segment arrays or none");
    *n_segs_out = 0;
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts, "null device pointer");
    const int64_t nb = (n_records + kSegThreads - 1) / kSegThreads;
    PALACE_REQUIRE(nb < (1ll << 31), "too many records");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_workspace(ctx, static_cast<size_t>(nb + 1) * sizeof(long long));
    if (rc) return rc;
    long long *sums = static_cast<long long *>(ctx->ws.ptr);
    hipLaunchKernelGGL(bam_seg_count_kernel, dim3(static_cast<unsigned>(nb)), dim3(kSegThreads), 0, ctx->stream, d_stream, d_starts, n_records, n_ref, sums);
    hipLaunchKernelGGL(bam_seg_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
    PALACE_HIP_TRY(hipGetLastError());
    long long n_segs = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&n_segs, sums + nb, sizeof n_segs, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_segs_out = n_segs;
    if (!emit || n_segs > cap) return PALACE_OK;                              // the count: the caller comes back with room
    hipLaunchKernelGGL(bam_seg_emit_kernel, dim3(static_cast<unsigned>(nb)), dim3(kSegThreads), 0, ctx->stream, d_stream, d_starts, n_records, n_ref,
                       sums, d_seg_tid, d_seg_pos, d_seg_len, cap);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
