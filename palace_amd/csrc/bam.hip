// The inflated BAM stream in HBM -> where its alignment records start (palace_bam_walk) and the match segments of the depth stage
// (palace_bam_match_segments): what `bamdepth --bam-gpu` needs to take a BAM without its records crossing PCIe again
// (include/palace_hip.h).  What a record IS -- the step of the walk, its CIGAR, spans, segments, aux fields, SA items -- is
// bam_record.hpp, the one text that the host loader (host/bam.cpp: BamLoad::walk, decode_range) compiles as well.
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
//
// For `generateGraph --bam-gpu` the same record starts feed the decode itself (what decode_range of host/bam.cpp does with the
// same functions, here one thread per record: a record's aux fields are a serial scan): palace_bam_columns writes the classify
// kernel's columns, palace_bam_sa_items parses the SA tags' text into palace_sa_item -- counted, scanned, emitted, as the segments are -- with the contig names looked up in a hash table
// built on the device from the header's names (palace_bam_names_create), palace_bam_name_keys re-keys the read names and
// palace_bam_names_differ compares them where they lie.  Every read lies inside the record the walk accepted.
#include "common.hpp"
#include "bam_record.hpp"
#include "bam_names.hpp"

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

// the guess's test: a step of the walk, and the fields a real record keeps in range
__device__ __forceinline__ bool looks_like_record(const uint8_t *d, int64_t p, int64_t total, int32_t n_ref, int64_t *next)
{
    if (walk_step(d, p, total, total, next) != 1) return false;
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
        if (walk_step(d, p, total, total, &next) != 1) { flags = kEnded; break; }
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

// ---- columns and SA items: decode_range's per-record columns (host/bam.cpp) ------------------------------------------------------

struct ColsOut {
    int32_t *tid, *pos, *mtid, *mpos, *nm, *ref_len, *read_len, *clip_s, *clip_e;
    uint16_t *flag;
    uint8_t *mapq;
    uint64_t *qkey;
};

constexpr int kColThreads = 256;

__global__ __launch_bounds__(kColThreads) void bam_columns_kernel(const uint8_t *d, const int64_t *starts, int64_t n, uint64_t seed, ColsOut o)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kColThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t s = starts[i], end = s + static_cast<int64_t>(ld32(d, s - 4));
    o.tid[i] = static_cast<int32_t>(ld32(d, s));
    o.pos[i] = static_cast<int32_t>(ld32(d, s + 4));
    o.mapq[i] = d[s + 9];
    o.flag[i] = static_cast<uint16_t>(ld16(d, s + 14));
    o.mtid[i] = static_cast<int32_t>(ld32(d, s + 20));
    o.mpos[i] = static_cast<int32_t>(ld32(d, s + 24));
    o.qkey[i] = name_key(d, s + 32, name_len(d, s), seed);
    const RecCigar c = record_cigar(d, s, end);
    const RecOps r = record_ops(d, s, c, false, [](int32_t, int32_t, int32_t) {});
    o.ref_len[i] = static_cast<int32_t>(r.ref_len);
    o.read_len[i] = static_cast<int32_t>(r.read_len);
    o.clip_s[i] = c.n_ops ? r.sc.clip_s() : -1;
    o.clip_e[i] = r.sc.clip_e();
    o.nm[i] = record_aux(d, c.aux, end).nm;
}

__global__ __launch_bounds__(kColThreads) void bam_name_keys_kernel(const uint8_t *d, const int64_t *starts, int64_t n, uint64_t seed, uint64_t *qkey)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kColThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t s = starts[i];
    qkey[i] = name_key(d, s + 32, name_len(d, s), seed);
}

// pairs of record ordinals whose C-string names differ (an ordinal outside [0, n) differs from everything: nothing is read for it)
__global__ __launch_bounds__(kColThreads) void bam_names_differ_kernel(const uint8_t *d, const int64_t *starts, int64_t n, const int64_t *pairs,
                                                                       int64_t n_pairs, unsigned long long *differ)
{
    const int64_t k = static_cast<int64_t>(blockIdx.x) * kColThreads + threadIdx.x;
    bool diff = false;
    if (k < n_pairs) {
        const int64_t a = pairs[2 * k], b = pairs[2 * k + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) diff = true;
        else if (a != b) {
            const int64_t sa = starts[a], sb = starts[b], la = name_len(d, sa);
            diff = la != name_len(d, sb);
            for (int64_t j = 0; !diff && j < la; j++) diff = d[sa + 32 + j] != d[sb + 32 + j];
        }
    }
    const unsigned long long m = __ballot(diff);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(differ, static_cast<unsigned long long>(__popcll(m)));
}

// (the table and its probe: bam_names.hpp)
// linear probing without removals: a name sits between its hash's slot and the first empty one (the table is at most half full)
__global__ __launch_bounds__(kColThreads) void bam_names_build_kernel(palace_bam_names t)
{
    const int32_t tid = static_cast<int32_t>(blockIdx.x * kColThreads + threadIdx.x);
    if (tid >= t.n_ref) return;
    const uint8_t *p = t.names + t.off[tid];
    const int64_t n = t.off[tid + 1] - t.off[tid];
    for (uint32_t at = hash_name(p, n) & t.mask;; at = (at + 1) & t.mask) {
        const int32_t old = atomicCAS(&t.slots[at], -1, tid);
        if (old < 0) return;
        if (is_name(t, old, p, n)) { atomicMax(&t.slots[at], tid); return; }
    }
}

__device__ __forceinline__ long long sa_items_of(const uint8_t *d, const int64_t *starts, int64_t i, int64_t n, int32_t n_ref)
{
    long long cnt = 0;
    if (i < n) record_sa_items(d, starts[i], n_ref, [&](const SaFields &) { cnt++; });
    return cnt;
}

__global__ __launch_bounds__(kSegThreads) void bam_sa_count_kernel(const uint8_t *d, const int64_t *starts, int64_t n, int32_t n_ref, long long *block_sum)
{
    __shared__ long long lds[kSegThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSegThreads + threadIdx.x;
    long long total;
    block_exclusive<long long, kSegThreads>(sa_items_of(d, starts, i, n, n_ref), lds, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSegThreads) void bam_sa_emit_kernel(const uint8_t *d, const int64_t *starts, int64_t n, palace_bam_names t,
                                                                  const long long *block_base, int32_t *sa_off, palace_sa_item *items, int64_t cap)
{
    __shared__ long long lds[kSegThreads / 64 + 1];
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kSegThreads + threadIdx.x;
    long long total;
    long long at = block_base[blockIdx.x] + block_exclusive<long long, kSegThreads>(sa_items_of(d, starts, i, n, t.n_ref), lds, &total);
    if (i >= n) return;
    sa_off[i] = static_cast<int32_t>(at);
    const int64_t s = starts[i];
    const int32_t own = static_cast<int32_t>(ld32(d, s));
    record_sa_items(d, s, t.n_ref, [&](const SaFields &f) {
        const palace_sa_item it = sa_item(d, f, [&](const uint8_t *name, int64_t n) { return is_name(t, own, name, n); },
                                          [&](const uint8_t *name, int64_t n) { return tid_of(t, name, n); });
        if (at < cap) items[at] = it;
        at++;
    });
    if (i == n - 1) sa_off[n] = static_cast<int32_t>(at);
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

extern "C" int palace_bam_columns(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                                  uint64_t key_seed, const palace_bam_cols *cols)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0 && cols, "bad argument");
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts, "null device pointer");
    PALACE_REQUIRE(cols->tid && cols->pos && cols->mtid && cols->mpos && cols->nm && cols->ref_len && cols->read_len && cols->clip_s && cols->clip_e &&
                   cols->flag && cols->mapq && cols->qkey, "a column is missing");
    const int64_t nb = (n_records + kColThreads - 1) / kColThreads;
    PALACE_REQUIRE(nb < (1ll << 31), "too many records");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    auto w = [](const int32_t *p) { return const_cast<int32_t *>(p); };
    const ColsOut o{w(cols->tid), w(cols->pos), w(cols->mtid), w(cols->mpos), w(cols->nm), w(cols->ref_len), w(cols->read_len), w(cols->clip_s),
                    w(cols->clip_e), const_cast<uint16_t *>(cols->flag), const_cast<uint8_t *>(cols->mapq), const_cast<uint64_t *>(cols->qkey)};
    hipLaunchKernelGGL(bam_columns_kernel, dim3(static_cast<unsigned>(nb)), dim3(kColThreads), 0, ctx->stream, d_stream, d_starts, n_records, key_seed, o);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bam_name_keys(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                                    uint64_t key_seed, uint64_t *d_qkey)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0, "bad argument");
    if (n_records == 0) return PALACE_OK;
    PALACE_REQUIRE(d_stream && d_starts && d_qkey, "null device pointer");
    const int64_t nb = (n_records + kColThreads - 1) / kColThreads;
    PALACE_REQUIRE(nb < (1ll << 31), "too many records");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bam_name_keys_kernel, dim3(static_cast<unsigned>(nb)), dim3(kColThreads), 0, ctx->stream, d_stream, d_starts, n_records, key_seed, d_qkey);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bam_names_differ(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                                       const int64_t *d_pairs, int64_t n_pairs, int64_t *n_differ_out)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0 && n_pairs >= 0 && n_differ_out, "bad argument");
    *n_differ_out = 0;
    if (n_pairs == 0) return PALACE_OK;
    PALACE_REQUIRE(d_pairs && (n_records == 0 || (d_stream && d_starts)), "null device pointer");
    const int64_t nb = (n_pairs + kColThreads - 1) / kColThreads;
    PALACE_REQUIRE(nb < (1ll << 31), "too many pairs");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    int rc = ensure_workspace(ctx, sizeof(unsigned long long));
    if (rc) return rc;
    unsigned long long *d_n = static_cast<unsigned long long *>(ctx->ws.ptr), n = 0;
    PALACE_HIP_TRY(hipMemsetAsync(d_n, 0, sizeof n, ctx->stream));
    hipLaunchKernelGGL(bam_names_differ_kernel, dim3(static_cast<unsigned>(nb)), dim3(kColThreads), 0, ctx->stream, d_stream, d_starts, n_records, d_pairs,
                       n_pairs, d_n);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    *n_differ_out = static_cast<int64_t>(n);
    return PALACE_OK;
}

extern "C" int palace_bam_names_create(palace_ctx *ctx, const uint8_t *d_names, const int64_t *d_name_off, int32_t n_ref, palace_bam_names **out)
{
    PALACE_REQUIRE(ctx && out && n_ref >= 0 && n_ref < (1 << 30), "bad argument");
    PALACE_REQUIRE(n_ref == 0 || (d_names && d_name_off), "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    uint32_t cap = 64;
    while (cap < 2u * static_cast<uint32_t>(n_ref)) cap <<= 1;
    palace_bam_names *t = new palace_bam_names{d_names, d_name_off, n_ref, cap - 1, nullptr};
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&t->slots), static_cast<size_t>(cap) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(t->slots, 0xff, static_cast<size_t>(cap) * sizeof(int32_t), ctx->stream);      // every slot -1
    if (e == hipSuccess && n_ref) {
        hipLaunchKernelGGL(bam_names_build_kernel, dim3((static_cast<unsigned>(n_ref) + kColThreads - 1) / kColThreads), dim3(kColThreads), 0, ctx->stream, *t);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        set_error("palace_bam_names_create: %s", hipGetErrorString(e));
        if (t->slots) (void)hipFree(t->slots);
        delete t;
        return PALACE_EHIP;
    }
    *out = t;
    return PALACE_OK;
}

extern "C" int palace_bam_names_destroy(palace_ctx *ctx, palace_bam_names *names)
{
    if (!names) return PALACE_OK;
    PALACE_REQUIRE(ctx, "bad argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (a look-up may still be running)
    PALACE_HIP_TRY(hipFree(names->slots));
    delete names;
    return PALACE_OK;
}

extern "C" int palace_bam_sa_items(palace_ctx *ctx, const uint8_t *d_stream, int64_t total, const int64_t *d_starts, int64_t n_records,
                                   const palace_bam_names *names, int32_t *d_sa_off, palace_sa_item *d_items, int64_t cap, int64_t *n_items_out)
{
    PALACE_REQUIRE(ctx && total >= 0 && n_records >= 0 && cap >= 0 && names && n_items_out, "bad argument");
    PALACE_REQUIRE(d_items || cap == 0, "items without room");
    *n_items_out = 0;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    if (n_records == 0) {
        if (d_sa_off) PALACE_HIP_TRY(hipMemsetAsync(d_sa_off, 0, sizeof(int32_t), ctx->stream));
        return PALACE_OK;
    }
    PALACE_REQUIRE(d_stream && d_starts, "null device pointer");
    const int64_t nb = (n_records + kSegThreads - 1) / kSegThreads;
    PALACE_REQUIRE(nb < (1ll << 31), "too many records");
    int rc = ensure_workspace(ctx, static_cast<size_t>(nb + 1) * sizeof(long long));
    if (rc) return rc;
    long long *sums = static_cast<long long *>(ctx->ws.ptr);
    hipLaunchKernelGGL(bam_sa_count_kernel, dim3(static_cast<unsigned>(nb)), dim3(kSegThreads), 0, ctx->stream, d_stream, d_starts, n_records, names->n_ref, sums);
    hipLaunchKernelGGL(bam_seg_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, sums, nb);
    PALACE_HIP_TRY(hipGetLastError());
    long long n_items = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&n_items, sums + nb, sizeof n_items, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    PALACE_REQUIRE(n_items <= 0x7fffffffll, "more SA items than sa_off's int32 can address");
    *n_items_out = n_items;
    if (!d_sa_off || n_items > cap) return PALACE_OK;                         // the count: the caller comes back with room
    hipLaunchKernelGGL(bam_sa_emit_kernel, dim3(static_cast<unsigned>(nb)), dim3(kSegThreads), 0, ctx->stream, d_stream, d_starts, n_records, *names, sums,
                       d_sa_off, d_items, cap);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
