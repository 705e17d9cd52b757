// filter_result's device half (include/palace_hip.h: palace_blast_groups .. palace_paths_first_of_equal; the rules: DESIGN.md 8):
// what the reference's filter_result.py decides, as integer problems over the BLAST table's text, the paths' record codes and one
// byte of bits per record.  The FASTA text itself is palace_final_fasta_lengths / _write with no separator (final_fasta.hip).
//
// The BLAST groups.  A wavefront owns a line, four lines to a workgroup, nothing shared between them: the lanes take the line 64
// bytes at a time, the TABs of a stretch are one ballot, the first four cuts go to the wave's words of LDS.  What the four columns
// MEAN is blast_line.hpp's.  Whether the line has the query and subject of the line before it is a compare of the two lines' bytes
// up to and with the second TAB, 64 at a time; no table of subjects exists.  A line leaves three things: whether it begins a
// group, what it adds to its group's sum (a line that begins a group by DIFFERING adds its length whatever its identity; the
// table's first line and every line inside a group add it when the identity passes), and -- a group's first line only -- the
// query's record.  Two scans (scan64.hpp) turn these into sums in front of every line and groups in front of every line, the
// groups' first lines are scattered by ordinal, and the last line of each group judges it: (double)sum / (double)length > ratio,
// an IEEE division.  A group may span any number of tiles and workgroups: nothing here knows of tiles.
//
// The plan.  A wavefront owns a path, its lanes stride the tokens: an OR of the records' bits and two sums, reduced by shuffles.
//
// First of equal.  A 64-bit hash of every code sequence (a sum over the tokens of mixed (code, position) words: integer, whatever
// the order of the lanes), cut to hash_bits, a stable palace_sort_u64; a path finds its run's begin by bisection and its leader --
// the first member of the run that equals it code by code, normally the first -- and takes, per class bit it has, a 32-bit
// atomicMin of its index at the leader.  Minima do not depend on order, and a collision costs compares, never the result.
#include "common.hpp"
#include "blast_line.hpp"
#include "fasta_names.hpp"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"     // (scan64.hpp's last_le is not used here)
#include "scan64.hpp"
#pragma clang diagnostic pop

namespace palace {
namespace {

constexpr int kLineThreads = 256, kLineWaves = kLineThreads / kWave;
constexpr int kClassBits = 6;

struct IdentityCuts { int64_t v[kBlastCuts]; };

static_assert(kBlastLineColumns == PALACE_BLAST_ECOLUMNS && kBlastLineEmptyName == PALACE_BLAST_ENAME && kBlastLineIdentity == PALACE_BLAST_EIDENTITY &&
              kBlastLineLength == PALACE_BLAST_ELENGTH && kBlastLineQuery == PALACE_BLAST_EQUERY && kBlastLineQueryEmpty == PALACE_BLAST_EQEMPTY,
              "the header states the codes");

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// ---- the BLAST table -----------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kLineThreads) void blast_lines_kernel(const uint8_t *t, const int64_t *start, int64_t n, palace_fasta_names names, IdentityCuts cut,
                                                                   int64_t *add, uint8_t *head, int32_t *qrec, unsigned long long *err)
{
    __shared__ int64_t s_cut[kLineWaves][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kLineWaves + wave;
    if (i >= n) return;                                                      // (uniform in the wave; no workgroup barrier below)
    const int64_t b = start[i], e = start[i + 1] - 1;
    volatile int64_t *L = s_cut[wave];
    int64_t tabs = 0;
    for (int64_t p = b; p < e && tabs < 4; p += kWave) {
        const int64_t q = p + lane;
        const bool tab = q < e && t[q] == '\t';
        const unsigned long long m = __ballot(tab);
        if (tab) {
            const int64_t ord = tabs + __popcll(m & lanes_below(lane));
            if (ord < 4) L[ord + 1] = q + 1;
        }
        tabs += __popcll(m);
    }
    __builtin_amdgcn_wave_barrier();
    int64_t c[5] = {b, 0, 0, 0, 0};
    for (int k = 1; k <= 4; k++) c[k] = k <= tabs ? L[k] : 0;
    const BlastLine l = blast_line_fields([t](int64_t at) { return static_cast<uint32_t>(t[at]); }, b, e, c, tabs);    // (every lane alike)
    int32_t code = l.error, r = -1;
    bool differs = false;
    if (!code && i > 0) {
        const int64_t pb = start[i - 1], pe = start[i] - 1, pre = c[2] - b;      // query TAB subject TAB: `pre` bytes
        if (pe - pb < pre) differs = true;
        else
            for (int64_t k0 = 0; k0 < pre && !differs; k0 += kWave) {
                const int64_t k = k0 + lane;
                differs = __ballot(k < pre && t[pb + k] != t[b + k]) != 0;
            }
    }
    const bool first = i == 0 || differs;
    if (!code && first) {
        r = record_of(names, t + b, c[1] - 1 - b);
        if (r < 0) code = kBlastLineQuery;
        else if (names.recs[r].length <= 0) code = kBlastLineQueryEmpty;
    }
    if (lane != 0) return;
    head[i] = first ? 1 : 0;
    qrec[i] = r;
    add[i] = (!code && (differs || blast_identity_passes(l, cut.v))) ? l.length : 0;
    if (code) atomicMin(err, static_cast<unsigned long long>(i + 1) << 8 | static_cast<unsigned long long>(code));
}

struct AddSize {
    const int64_t *add;
    __device__ __forceinline__ long long operator()(int64_t i) const { return add[i]; }
};
struct HeadSize {
    const uint8_t *head;
    __device__ __forceinline__ long long operator()(int64_t i) const { return head[i]; }
};

// gord[i]: the groups that begin in front of line i; a group's first line says where the group begins
__global__ __launch_bounds__(256) void blast_group_start_kernel(const uint8_t *head, const int64_t *gord, int64_t n, int64_t *gstart)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n && head[i]) gstart[gord[i]] = i;
}

// a group's last line judges it.  Several groups may flag one record: they all store the same byte
__global__ __launch_bounds__(256) void blast_verdict_kernel(const uint8_t *head, const int64_t *gord, const int64_t *gstart, const int64_t *cum, const int32_t *qrec,
                                                            int64_t n, const palace_fasta_rec *recs, double ratio, uint8_t *seg)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= n || (i + 1 < n && !head[i + 1])) return;
    const int64_t s = gstart[gord[i] + head[i] - 1];
    const int32_t r = qrec[s];
    if (static_cast<double>(cum[i + 1] - cum[s]) / static_cast<double>(recs[r].length) > ratio) seg[r] = 1;
}

__global__ __launch_bounds__(256) void count_bytes_kernel(const uint8_t *v, int64_t n, unsigned long long *count)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const unsigned long long m = __ballot(i < n && v[i] != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, static_cast<unsigned long long>(__popcll(m)));
}

// ---- the paths' classes ----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool is_found(int32_t c) { return c >= 0 && (c & PALACE_PATH_SECOND_TRY) == 0; }

__global__ __launch_bounds__(kLineThreads) void filter_plan_kernel(const int32_t *code, const int64_t *path_off, int64_t n_paths, const uint8_t *tag,
                                                                   const palace_fasta_rec *recs, const uint8_t *rec_bits, uint8_t *cls, int64_t *all_len)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kLineWaves + (threadIdx.x >> 6);
    if (p >= n_paths) return;
    const int64_t a = path_off[p], L = path_off[p + 1] - a;
    uint32_t bits = 0;
    long long all = 0, hit = 0;
    for (int64_t k = lane; k < L; k += kWave) {
        const int32_t c = code[a + k];
        if (!is_found(c)) continue;
        const long long len = recs[c >> 2].length;
        const uint32_t rb = rec_bits[c >> 2];
        bits |= rb;
        all += len;
        if (rb & PALACE_FILTERRES_REC_BLAST) hit += len;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        bits |= __shfl_xor(bits, d, 64);
        all += __shfl_xor(all, d, 64);
        hit += __shfl_xor(hit, d, 64);
    }
    if (lane != 0) return;
    const bool gene = bits & PALACE_FILTERRES_REC_GENE, s07 = bits & PALACE_FILTERRES_REC_S07, s09 = bits & PALACE_FILTERRES_REC_S09;
    uint32_t out = 0;
    if (L == 1 && (tag[p] & PALACE_FILTERRES_TAG_SELF)) out = (gene || s07) ? PALACE_FILTERRES_SELFGENE : (PALACE_FILTERRES_WRITE | PALACE_FILTERRES_PLAIN);
    else if (L > 0) {
        if (tag[p] & PALACE_FILTERRES_TAG_CYCLE) out |= (gene ? PALACE_FILTERRES_CYCLEGENE : 0) | (s09 ? PALACE_FILTERRES_CYCLESCORE : 0);
        const bool flags = gene || (all != 0 && static_cast<double>(hit) / static_cast<double>(all) > 0.2);
        if (flags || (s09 && all >= 1000)) out |= PALACE_FILTERRES_WRITE | ((gene && s09) ? PALACE_FILTERRES_GENESCORE : 0);
    }
    cls[p] = static_cast<uint8_t>(out);
    all_len[p] = all;
}

// ---- the first of equal paths ------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull; x ^= x >> 27; x *= 0x94d049bb133111ebull; x ^= x >> 31;
    return x;
}

__global__ __launch_bounds__(kLineThreads) void path_hash_kernel(const int32_t *code, const int64_t *path_off, int64_t n_paths, uint64_t mask, uint64_t *key)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * kLineWaves + (threadIdx.x >> 6);
    if (p >= n_paths) return;
    const int64_t a = path_off[p], L = path_off[p + 1] - a;
    uint64_t h = 0;
    for (int64_t k = lane; k < L; k += kWave)
        h += mix64((static_cast<uint64_t>(static_cast<uint32_t>(code[a + k])) << 32 | static_cast<uint64_t>(k & 0xffffffff)) + 0x9e3779b97f4a7c15ull);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) h += __shfl_xor(h, d, 64);
    if (lane == 0) key[p] = mix64(h + static_cast<uint64_t>(L)) & mask;
}

__device__ __forceinline__ bool same_codes(const int32_t *code, const int64_t *path_off, int64_t p, int64_t q)
{
    const int64_t a = path_off[p], b = path_off[q], L = path_off[p + 1] - a;
    if (path_off[q + 1] - b != L) return false;
    for (int64_t k = 0; k < L; k++)
        if (code[a + k] != code[b + k]) return false;
    return true;
}

// key / perm: the hashes sorted, stably, so the members of a run lie in path order and the first equal one is the smallest
__global__ __launch_bounds__(256) void path_leader_kernel(const uint64_t *key, const uint32_t *perm, int64_t n, const int32_t *code, const int64_t *path_off,
                                                          const uint8_t *cls, uint32_t *leader, uint32_t *first)
{
    const int64_t s = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (s >= n) return;
    const uint64_t k = key[s];
    int64_t lo = 0, hi = s;                                                  // the first entry with this key
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (key[mid] < k) lo = mid + 1; else hi = mid;
    }
    const uint32_t p = perm[s];
    uint32_t q = p;
    for (int64_t m = lo; m < s; m++)
        if (same_codes(code, path_off, p, perm[m])) { q = perm[m]; break; }
    leader[p] = q;
    for (int c = 0; c < kClassBits; c++)
        if (cls[p] >> c & 1) atomicMin(&first[c * n + q], p);
}

__global__ __launch_bounds__(256) void path_first_kernel(const uint8_t *cls, const uint32_t *leader, const uint32_t *first, int64_t n, uint8_t *out)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p >= n) return;
    uint32_t v = 0;
    for (int c = 0; c < kClassBits; c++)
        if ((cls[p] >> c & 1) && first[c * n + leader[p]] == static_cast<uint32_t>(p)) v |= 1u << c;
    out[p] = static_cast<uint8_t>(v);
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_blast_identity_cuts(double threshold, int64_t *cut)
{
    PALACE_REQUIRE(cut, "bad argument");
    blast_identity_cuts(threshold, cut);
    return PALACE_OK;
}

extern "C" int palace_blast_groups(palace_ctx *ctx, const uint8_t *d_text, const int64_t *d_line_start, int64_t n_lines, const palace_fasta_names *names,
                                   int64_t n_records, double blast_ratio, const int64_t *cut, uint8_t *d_seg, int64_t *out)
{
    PALACE_REQUIRE(ctx && names && cut && out && n_lines >= 0 && n_lines < (1ll << 29) && n_records == names->n, "bad argument (lines < 2^29, the table's records)");
    PALACE_REQUIRE((n_records == 0 || d_seg) && (n_lines == 0 || (d_text && d_line_start)), "null device pointer");
    out[0] = n_lines;
    out[1] = out[2] = out[3] = out[4] = 0;
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    if (n_records) PALACE_HIP_TRY(hipMemsetAsync(d_seg, 0, static_cast<size_t>(n_records), ctx->stream));
    if (n_lines == 0) return PALACE_OK;
    const size_t n = static_cast<size_t>(n_lines);
    const size_t b_add = align256(n * 8), b_cum = align256((n + 1) * 8), b_qrec = align256(n * 4), b_head = align256(n);
    const size_t at_sums = b_add + 2 * b_cum + b_add + b_qrec + b_head;
    const int rc = ensure_workspace(ctx, at_sums + scan_sizes_bytes(n_lines));
    if (rc) return rc;
    uint8_t *w = static_cast<uint8_t *>(ctx->ws.ptr);
    int64_t *add = reinterpret_cast<int64_t *>(w), *cum = reinterpret_cast<int64_t *>(w + b_add), *gord = reinterpret_cast<int64_t *>(w + b_add + b_cum),
            *gstart = reinterpret_cast<int64_t *>(w + b_add + 2 * b_cum);
    int32_t *qrec = reinterpret_cast<int32_t *>(w + b_add + 2 * b_cum + b_add);
    uint8_t *head = w + b_add + 2 * b_cum + b_add + b_qrec;
    unsigned long long *small = reinterpret_cast<unsigned long long *>(ctx->d_small), got[2] = {~0ull, 0};
    PALACE_HIP_TRY(hipMemcpyAsync(small, got, sizeof got, hipMemcpyHostToDevice, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));                       // (got is this call's own)
    IdentityCuts cuts;
    for (int k = 0; k < kBlastCuts; k++) cuts.v[k] = cut[k];
    hipLaunchKernelGGL(blast_lines_kernel, dim3(static_cast<unsigned>((n_lines + kLineWaves - 1) / kLineWaves)), dim3(kLineThreads), 0, ctx->stream, d_text,
                       d_line_start, n_lines, *names, cuts, add, head, qrec, small);
    PALACE_HIP_TRY(hipGetLastError());
    PALACE_HIP_TRY(hipMemcpyAsync(got, small, sizeof(got[0]), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (got[0] != ~0ull) {                                                   // a faulty table has no groups
        out[3] = static_cast<int64_t>(got[0] >> 8);
        out[4] = static_cast<int64_t>(got[0] & 0xff);
        return PALACE_OK;
    }
    scan_sizes_into(ctx, AddSize{add}, n_lines, cum, reinterpret_cast<long long *>(w + at_sums));
    scan_sizes_into(ctx, HeadSize{head}, n_lines, gord, reinterpret_cast<long long *>(w + at_sums));
    const dim3 lines(static_cast<unsigned>((n_lines + 255) / 256));
    hipLaunchKernelGGL(blast_group_start_kernel, lines, dim3(256), 0, ctx->stream, head, gord, n_lines, gstart);
    hipLaunchKernelGGL(blast_verdict_kernel, lines, dim3(256), 0, ctx->stream, head, gord, gstart, cum, qrec, n_lines, names->recs, blast_ratio, d_seg);
    hipLaunchKernelGGL(count_bytes_kernel, dim3(static_cast<unsigned>((n_records + 255) / 256 + 1)), dim3(256), 0, ctx->stream, d_seg, n_records, small + 1);
    PALACE_HIP_TRY(hipGetLastError());
    long long groups = 0;
    PALACE_HIP_TRY(hipMemcpyAsync(&groups, gord + n_lines, sizeof groups, hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipMemcpyAsync(got + 1, small + 1, sizeof(got[1]), hipMemcpyDeviceToHost, ctx->stream));
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    out[1] = groups;
    out[2] = static_cast<int64_t>(got[1]);
    return PALACE_OK;
}

extern "C" int palace_filter_result_plan(palace_ctx *ctx, const int32_t *d_code, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_tag,
                                         const palace_fasta_rec *d_recs, const uint8_t *d_rec_bits, uint8_t *d_class, int64_t *d_all_len)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && n_paths < (1ll << 31), "bad argument (paths < 2^31)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_tag && d_class && d_all_len, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(filter_plan_kernel, dim3(static_cast<unsigned>((n_paths + kLineWaves - 1) / kLineWaves)), dim3(kLineThreads), 0, ctx->stream, d_code,
                       d_path_off, n_paths, d_tag, d_recs, d_rec_bits, d_class, d_all_len);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_paths_first_of_equal(palace_ctx *ctx, const int32_t *d_code, const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_class,
                                           int32_t hash_bits, uint8_t *d_first)
{
    PALACE_REQUIRE(ctx && n_paths >= 0 && n_paths < (1ll << 31) && hash_bits >= 0 && hash_bits <= 64, "bad argument (paths < 2^31, hash_bits 0 .. 64)");
    if (n_paths == 0) return PALACE_OK;
    PALACE_REQUIRE(d_path_off && d_class && d_first, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t n = static_cast<size_t>(n_paths), sort_bytes = palace_sort_u64_scratch_bytes(n_paths);
    const size_t b_key = align256(n * 8), b_perm = align256(n * 4), b_first = align256(n * 4 * kClassBits);
    const int rc = ensure_workspace(ctx, b_key + 2 * b_perm + b_first + sort_bytes + 256);
    if (rc) return rc;
    uint8_t *w = static_cast<uint8_t *>(ctx->ws.ptr);
    uint64_t *key = reinterpret_cast<uint64_t *>(w);
    uint32_t *perm = reinterpret_cast<uint32_t *>(w + b_key), *leader = reinterpret_cast<uint32_t *>(w + b_key + b_perm),
             *first = reinterpret_cast<uint32_t *>(w + b_key + 2 * b_perm);
    void *sort_scratch = w + b_key + 2 * b_perm + b_first;
    const uint64_t mask = hash_bits == 64 ? ~0ull : (1ull << hash_bits) - 1ull;
    PALACE_HIP_TRY(hipMemsetAsync(first, 0xff, n * 4 * kClassBits, ctx->stream));
    hipLaunchKernelGGL(path_hash_kernel, dim3(static_cast<unsigned>((n_paths + kLineWaves - 1) / kLineWaves)), dim3(kLineThreads), 0, ctx->stream, d_code, d_path_off,
                       n_paths, mask, key);
    PALACE_HIP_TRY(hipGetLastError());
    const int src = palace_sort_u64(ctx, key, perm, n_paths, hash_bits, sort_scratch, sort_bytes);
    if (src) return src;
    const dim3 paths(static_cast<unsigned>((n_paths + 255) / 256));
    hipLaunchKernelGGL(path_leader_kernel, paths, dim3(256), 0, ctx->stream, key, perm, n_paths, d_code, d_path_off, d_class, leader, first);
    hipLaunchKernelGGL(path_first_kernel, paths, dim3(256), 0, ctx->stream, d_class, leader, first, n_paths, d_first);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
