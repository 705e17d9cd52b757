// FASTQ text in HBM -> the ASCII read set of palace_eref_count_reads (include/palace_hip.h: palace_fastq_parse), and the CRC-32
// of inflated BGZF members (palace_crc32_members): what eref needs to take a compressed FASTQ without its text crossing PCIe.
//
// The parser has the getline semantics of the host's (host/fastx.hpp: plan_fastq / extract_fastq_part): a line ends at '\n' only,
// a sequence line is a line whose 0-based index is 1 mod 4, its bytes are copied unchanged.  A window of text is three launches:
//   1. counts: a tile of 4096 bytes (256 lanes x 16) counts its newlines and, by the line phase relative to the tile's start
//      (newlines before the byte, mod 4), its newlines and its other bytes -- the host's n_by_phase / bytes_by_phase;
//   2. scan: one workgroup fixes every tile's line phase, first read and first base from the cursor and the counts, and moves the
//      cursor past the window (closing an unterminated last line when the window is the file's last);
//   3. scatter: every lane finds its bytes' phases again, a workgroup scan places its sequence bytes and read ends.
// A line may run over any number of windows: the cursor carries its index and whether it has begun, not its text.
#include "common.hpp"
#include "text_lanes.hpp"

namespace palace {
namespace {

constexpr int kTileThreads = 256, kTileBytes = kTileThreads * kLaneBytes;
constexpr int kScanThreads = 1024;

// per tile, written by the counts kernel: newlines, and for the relative phases r = 0..3 (16 bits each) the newlines and the
// other bytes that have r mod 4 newlines of the tile in front of them; written by the scan kernel: the tile's place
struct TileCounts { uint32_t nl; uint32_t pad; uint64_t nl_rel, bytes_rel; };
struct TileBase { int64_t read0, byte0; int32_t phase, pad; };
struct ScratchHead { int32_t skip; int32_t pad[15]; };

inline size_t tiles_of(int64_t n) { return static_cast<size_t>((n + kTileBytes - 1) / kTileBytes); }

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int s) { return s ? (x << s) | (x >> (64 - s)) : x; }

// counters by relative phase: field (j & 3) of 16 bits
__device__ __forceinline__ void lane_counts(const uint32_t w[4], int valid, uint32_t nlm, uint64_t &nl_rel, uint64_t &bytes_rel)
{
    nl_rel = 0; bytes_rel = 0;
    int j = 0;
#pragma unroll
    for (int k = 0; k < kLaneBytes; k++) {
        const uint64_t one = 1ull << (16 * (j & 3));
        const bool nl = (nlm >> k) & 1u;
        if (k < valid) { if (nl) nl_rel += one; else bytes_rel += one; }
        j += nl;
    }
}

__global__ __launch_bounds__(kTileThreads) void fastq_counts_kernel(const uint8_t *text, int64_t n, TileCounts *tiles)
{
    __shared__ uint32_t s_nl[kTileThreads / 64 + 1];
    __shared__ unsigned long long s_red[2][kTileThreads / 64];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    const uint32_t nlm = newline_mask(w, valid);
    uint32_t nl_total;
    const uint32_t j0 = block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(nlm)), s_nl, &nl_total);
    uint64_t nr, br;
    lane_counts(w, valid, nlm, nr, br);
    nr = rotl64(nr, 16 * (j0 & 3)); br = rotl64(br, 16 * (j0 & 3));     // relative to the tile's first byte
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { nr += __shfl_xor(nr, d, 64); br += __shfl_xor(br, d, 64); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_red[0][wave] = nr; s_red[1][wave] = br; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t a = 0, b = 0;
        for (int k = 0; k < kTileThreads / 64; k++) { a += s_red[0][k]; b += s_red[1][k]; }
        tiles[blockIdx.x] = TileCounts{nl_total, 0u, a, b};
    }
}

__device__ __forceinline__ int64_t field(uint64_t packed, int r) { return static_cast<int64_t>((packed >> (16 * (r & 3))) & 0xffffu); }

// one workgroup: tiles' places, the cursor moved past the window
__global__ __launch_bounds__(kScanThreads) void fastq_scan_kernel(const uint8_t *text, int64_t n, int64_t n_tiles, int final_window,
                                                                  palace_fastq_cursor *cur, const TileCounts *tiles, TileBase *bases,
                                                                  ScratchHead *head, int64_t *offsets, int64_t bases_cap, int64_t offsets_cap)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    const palace_fastq_cursor c = *cur;
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t t0 = threadIdx.x * per, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    long long nl = 0;
    for (int64_t t = t0; t < t1; t++) nl += tiles[t].nl;
    long long nl_total;
    const long long line0 = c.line + block_exclusive<long long, kScanThreads>(nl, s_scan, &nl_total);
    long long reads = 0, bytes = 0;
    {
        long long line = line0;
        for (int64_t t = t0; t < t1; t++) {
            const TileCounts k = tiles[t];
            const int r = static_cast<int>((1 - line) & 3);                   // relative phase of the sequence lines in this tile
            reads += field(k.nl_rel, r); bytes += field(k.bytes_rel, r);
            line += k.nl;
        }
    }
    long long reads_total, bytes_total;
    const long long read0 = c.reads + block_exclusive<long long, kScanThreads>(reads, s_scan, &reads_total);
    const long long byte0 = c.bases + block_exclusive<long long, kScanThreads>(bytes, s_scan, &bytes_total);
    {
        long long line = line0, rd = read0, by = byte0;
        for (int64_t t = t0; t < t1; t++) {
            const TileCounts k = tiles[t];
            const int r = static_cast<int>((1 - line) & 3);
            bases[t] = TileBase{rd, by, static_cast<int32_t>(line & 3), 0};
            rd += field(k.nl_rel, r); by += field(k.bytes_rel, r);
            line += k.nl;
        }
    }
    if (threadIdx.x == 0) {
        palace_fastq_cursor o = c;
        o.line = c.line + nl_total;
        o.reads = c.reads + reads_total;
        o.bases = c.bases + bytes_total;
        o.open = n > 0 ? (text[n - 1] != '\n') : c.open;
        const bool close = final_window && o.open;                        // a last line without '\n' is a line
        const bool close_read = close && (o.line & 3) == 1;
        const int64_t reads_after = o.reads + (close_read ? 1 : 0);
        if (c.error || o.bases > bases_cap || reads_after + 1 > offsets_cap) {
            head->skip = 1;                                                 // nothing of this window is written
            if (!c.error) cur->error = 1;
            return;
        }
        head->skip = 0;
        if (close_read) offsets[reads_after] = o.bases;
        if (close) { o.line++; o.open = 0; }
        o.reads = reads_after;
        *cur = o;
    }
}

__global__ __launch_bounds__(kTileThreads) void fastq_scatter_kernel(const uint8_t *text, int64_t n, const TileBase *tbase,
                                                                     const ScratchHead *head, uint8_t *out_bases, int64_t *offsets)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    if (head->skip) return;                                                  // (uniform)
    const TileBase tb = tbase[blockIdx.x];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    const uint32_t nlm = newline_mask(w, valid);
    uint32_t tot;
    const uint32_t j0 = block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(nlm)), s_scan, &tot);
    // the lane's sequence bytes and read ends: bytes whose line phase is 1
    const int ph0 = static_cast<int>((tb.phase + j0) & 3);
    uint32_t seq = 0, ends = 0;                                              // bit k: byte k is a sequence byte / ends a read
    {
        int ph = ph0;
#pragma unroll
        for (int k = 0; k < kLaneBytes; k++) {
            const bool nl = (nlm >> k) & 1u;
            if (k < valid && ph == 1) { if (nl) ends |= 1u << k; else seq |= 1u << k; }
            ph = (ph + nl) & 3;
        }
    }
    const uint32_t mine = static_cast<uint32_t>(__popc(seq)) | (static_cast<uint32_t>(__popc(ends)) << 16);
    const uint32_t before = block_exclusive<uint32_t, kTileThreads>(mine, s_scan, &tot);
    int64_t pos = tb.byte0 + (before & 0xffffu), rd = tb.read0 + (before >> 16);
    if (!(seq | ends)) return;
#pragma unroll
    for (int k = 0; k < kLaneBytes; k++) {
        if ((seq >> k) & 1u) out_bases[pos++] = static_cast<uint8_t>(byte_of(w, k));
        else if ((ends >> k) & 1u) offsets[++rd] = pos;
    }
}

// ---- CRC-32 (the gzip polynomial, reflected) of members, one wavefront each ----------------------------------------------------
constexpr uint32_t kPoly = 0xedb88320u;

// a(x) * b(x) mod P(x), reflected (zlib's multmodp)
__device__ uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        b = (b & 1) ? (b >> 1) ^ kPoly : b >> 1;
    }
    return p;
}
// x^(8 n) mod P(x), from x2n[k] = x^(2^k)
__device__ uint32_t x8nmodp(const uint32_t *x2n, uint32_t n)
{
    uint32_t p = 1u << 31;                                                   // x^0
    for (int k = 3; n; n >>= 1, k++)
        if (n & 1) p = multmodp(x2n[k & 31], p);
    return p;
}

__global__ __launch_bounds__(64) void crc32_members_kernel(const uint8_t *data, int64_t n_members, const int64_t *off, const int32_t *len,
                                                           uint32_t *crc_out)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t x2n[32];
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = static_cast<uint32_t>(i);
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kPoly : c >> 1;
        tab[i] = c;
    }
    if (lane == 0) {
        uint32_t p = 1u << 30;                                               // x^1
        x2n[0] = p;
        for (int k = 1; k < 32; k++) x2n[k] = p = multmodp(p, p);
    }
    __syncthreads();
    const int64_t m = blockIdx.x;
    const int32_t L = len[m] > 0 ? len[m] : 0;
    const uint8_t *src = data + off[m];
    // lane l: bytes [l * S, min(L, (l + 1) * S))
    const int32_t S = (L + 63) / 64;
    const int32_t a = lane * S < L ? lane * S : L, b = a + S < L ? a + S : L;
    uint32_t c = ~0u;
    int32_t i = a;
    for (; i < b && ((reinterpret_cast<uintptr_t>(src + i) & 3) != 0); i++) c = tab[(c ^ src[i]) & 0xff] ^ (c >> 8);
    for (; i + 4 <= b; i += 4) {                                           // aligned dwords
        const uint32_t v = *reinterpret_cast<const uint32_t *>(src + i);
        c ^= v;
        c = tab[c & 0xff] ^ (c >> 8);
        c = tab[c & 0xff] ^ (c >> 8);
        c = tab[c & 0xff] ^ (c >> 8);
        c = tab[c & 0xff] ^ (c >> 8);
    }
    for (; i < b; i++) c = tab[(c ^ src[i]) & 0xff] ^ (c >> 8);
    uint32_t crc = ~c;
    uint32_t n = static_cast<uint32_t>(b - a);
    // crc(A B) = crc(A) x^(8 |B|) + crc(B): lanes combined pairwise, lane 0 ends with the member's
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t oc = __shfl_down(crc, d, 64), on = __shfl_down(n, d, 64);
        if ((lane & (2 * d - 1)) == 0 && lane + d < 64) {
            crc = multmodp(x8nmodp(x2n, on), crc) ^ oc;
            n += on;
        }
    }
    if (lane == 0) crc_out[m] = crc;
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_fastq_scratch_bytes(int64_t max_window)
{
    const size_t t = tiles_of(max_window < 0 ? 0 : max_window);
    return align256(sizeof(ScratchHead)) + align256(t * sizeof(TileCounts)) + align256(t * sizeof(TileBase));
}

extern "C" int palace_fastq_parse(palace_ctx *ctx, const uint8_t *d_text, int64_t n, int final_window, palace_fastq_cursor *d_cursor,
                                  uint8_t *d_bases, int64_t bases_cap, int64_t *d_offsets, int64_t offsets_cap, void *d_scratch,
                                  size_t scratch_bytes)
{
    PALACE_REQUIRE(ctx && n >= 0 && bases_cap >= 0 && offsets_cap >= 1, "bad argument");
    PALACE_REQUIRE(d_cursor && d_offsets && d_scratch && (d_bases || bases_cap == 0) && (d_text || n == 0), "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15) == 0, "the text must be 16-byte aligned");
    PALACE_REQUIRE(scratch_bytes >= palace_fastq_scratch_bytes(n), "scratch smaller than palace_fastq_scratch_bytes(n)");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t nt = tiles_of(n);
    uint8_t *s = static_cast<uint8_t *>(d_scratch);
    ScratchHead *head = reinterpret_cast<ScratchHead *>(s);
    TileCounts *counts = reinterpret_cast<TileCounts *>(s + align256(sizeof(ScratchHead)));
    TileBase *tb = reinterpret_cast<TileBase *>(s + align256(sizeof(ScratchHead)) + align256(nt * sizeof(TileCounts)));
    if (nt) hipLaunchKernelGGL(fastq_counts_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, n, counts);
    hipLaunchKernelGGL(fastq_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_text, n, static_cast<int64_t>(nt), final_window,
                       d_cursor, counts, tb, head, d_offsets, bases_cap, offsets_cap);
    if (nt) hipLaunchKernelGGL(fastq_scatter_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, n, tb, head,
                               d_bases, d_offsets);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_crc32_members(palace_ctx *ctx, const uint8_t *d_data, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                                    uint32_t *d_crc)
{
    PALACE_REQUIRE(ctx && n_members >= 0 && n_members < (1ll << 31), "bad argument");
    if (n_members == 0) return PALACE_OK;
    PALACE_REQUIRE(d_data && d_off && d_len && d_crc, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(crc32_members_kernel, dim3(static_cast<unsigned>(n_members)), dim3(64), 0, ctx->stream, d_data, n_members, d_off, d_len,
                       d_crc);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
