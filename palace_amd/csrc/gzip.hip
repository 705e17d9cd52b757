// A gzip member that is not BGZF, inflated on the device: ONE DEFLATE stream decoded by many wavefronts.
//
// bgzf_inflate_kernel (inflate.hip) has a wavefront per member; a file written by gzip or pigz is one member, so the parallelism has
// to come from inside the stream.  DEFLATE offers two handles: a block can be decoded from its first bit by whoever knows where that
// bit is, and the only thing such a decoder lacks is the 32 KiB of text before it.  Hence two passes (the method of pugz and
// rapidgzip, restated for a wavefront):
//   find     every `stride` compressed bytes, the first bit position at which a non-final dynamic-Huffman block header parses
//            completely.  Lanes filter candidate positions (block type, HLIT / HDIST, a complete code-length code: 74 bits and a
//            Kraft sum), the wave validates the survivors with the decoder's own read_block_codes.
//   size     a wave per candidate chunk decodes without writing: output length and end bit do not depend on the unknown window.
//   (host)   the chain: a chunk counts when it starts where its predecessor ended; positions nobody found are queued and sized alone.
//   decode   a wave per chunk on the chain writes 16-bit symbols: a literal, or 0x8000 | k = "byte k of the 32 KiB before me".
//   chain    ONE workgroup walks the chunks in order with the running window in LDS and leaves every chunk's starting window in HBM.
//   resolve  every symbol becomes its byte, references through the chunk's window; then CRC-32 per chunk (fastq.hip), combined per
//            member on the host.
//
// Most waves of find and size run on positions nobody has confirmed and decode garbage by design.  Memory safety does not depend on
// the input: input dwords are fetched only inside the span's buffer (zeros beyond), every LDS index is masked, the size pass writes
// nothing and ends with the buffer (every symbol consumes a bit), the decode pass writes only below the length the size pass
// found, and references are masked to the window.  No workgroup waits for another.
#include <zlib.h>

#include <algorithm>
#include <chrono>

#include "common.hpp"
#include "deflate.hpp"
#include "../host/gzip_member.hpp"

namespace palace {

constexpr int kGzWindow = 32768;                 // DEFLATE's window
constexpr uint16_t kGzMarker = 0x8000;           // symbol = kGzMarker | index into the window before the chunk
constexpr int kGzMaxRounds = 16;                 // certain starts queued per span behind the first size pass
constexpr int64_t kGzMaxBatchChunks = 4096;      // windows in HBM: 128 MiB

using palace_host::GzChunk;
using palace_host::GzResult;
static_assert(palace_host::kGzOk == kInfOk && palace_host::kGzNeedsInput == kInfInput, "the host's chain walk reads the decoder's status");
constexpr int64_t kGzFarBits = 8ll << 20;        // a chunk ends within a block of its stop: 1 MiB of compressed data behind it is no chunk
constexpr int32_t kInfFar = 7;

// Decode from c.start to the first block boundary at or after c.stop or behind a final block.  kWrite: the symbols go to `out`
// (c.out_len of them, not one more); otherwise they are counted.
template <bool kWrite>
__device__ __forceinline__ GzResult inflate_chunk(const uint32_t *in, int64_t n_bytes, const GzChunk &c, uint16_t *out, CodeTables &t)
{
    const int lane = threadIdx.x & 63;
    const Code lit{t.lit_primary, t.lit_sorted, t.lit_count, kLitBits}, dist{t.dist_primary, t.dist_sorted, t.dist_count, kDistBits},
               pre{t.pre_primary, t.pre_sorted, t.pre_count, 7};
    const int64_t end_bit = n_bytes * 8;
    BitReader br;
    br.base = in;
    br.last = n_bytes > 0 ? (n_bytes - 1) >> 2 : -1;
    int64_t opos = 0, reach = 0;
    int32_t err = kInfOk;
    bool fin = false;
    if (c.start < 0 || c.start >= end_bit) return GzResult{0, c.start, 0, kInfInput, 0};
    const int64_t far = c.stop < end_bit - kGzFarBits ? c.stop + kGzFarBits : end_bit + 128;
    br.seek(c.start);
    auto written = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); };
    auto back = [&](int64_t at) { return __hip_atomic_load(out + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    while (!fin && br.bit_pos() < c.stop) {
        if (br.bit_pos() + 3 > end_bit) { err = kInfInput; break; }
        br.refill();
        fin = br.take(1) != 0;
        const uint32_t btype = br.take(2);
        if (btype == 0) {
            const int64_t p_bit = (br.bit_pos() + 7) & ~7ll;
            if (p_bit + 32 > end_bit) { err = kInfInput; break; }
            br.seek(p_bit);
            br.refill();
            const uint32_t len = br.take(16);
            br.refill();
            const uint32_t nlen = br.take(16);
            if ((len ^ 0xffffu) != nlen) { err = kInfBadBlock; break; }
            const int64_t data_bit = p_bit + 32;
            if (data_bit + static_cast<int64_t>(len) * 8 > end_bit) { err = kInfInput; break; }
            if (kWrite) {
                if (static_cast<int64_t>(len) > c.out_len - opos) { err = kInfOverrun; break; }
                const uint8_t *src = reinterpret_cast<const uint8_t *>(in) + (data_bit >> 3);
                for (uint32_t i = lane; i < len; i += 64) out[opos + i] = src[i];
            }
            opos += len;
            br.seek(data_bit + static_cast<int64_t>(len) * 8);
            continue;
        }
        if (btype == 3) { err = kInfBadBlock; break; }
        err = read_block_codes(btype, br, t.lens, pre, lit, dist);
        if (err != kInfOk) break;
        for (;;) {
            br.refill();
            if (br.bit_pos() > end_bit + 64) { err = kInfInput; break; }       // every symbol consumes a bit: the loop ends with the buffer
            if (br.bit_pos() > far) { err = kInfFar; break; }                  // ... and, for a start that was no start, long before that
            const int sym = decode_sym(lit, br);
            if (sym < 0) { err = kInfBadCode; break; }
            if (sym < 256) {
                if (kWrite) {
                    if (opos >= c.out_len) { err = kInfOverrun; break; }
                    if (lane == 0) out[opos] = static_cast<uint16_t>(sym);
                }
                opos++;
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) { err = kInfBadCode; break; }
            int32_t lbase, dbase;
            int lextra, dextra;
            len_code(sym - 257, lbase, lextra);
            const int32_t len = lbase + static_cast<int32_t>(br.take(lextra));
            br.refill();
            const int ds = decode_sym(dist, br);
            if (ds < 0 || ds > 29) { err = kInfBadDistance; break; }
            br.refill();
            dist_code(ds, dbase, dextra);
            const int32_t d = dbase + static_cast<int32_t>(br.take(dextra));    // <= 32768
            if (d > opos) {                                                    // before the chunk: known to the window alone, counted here
                if (c.first) { err = kInfBadDistance; break; }                 // ... and before the start of the member
                if (d - opos > reach) reach = d - opos;
            }
            if (kWrite) {
                if (len > c.out_len - opos) { err = kInfOverrun; break; }
                written();
                for (int32_t i = lane; i < len; i += 64) {
                    const int32_t s = d >= len ? i : i % d;
                    const int64_t at = opos - d + s;                           // >= -32768
                    out[opos + i] = at >= 0 ? back(at) : static_cast<uint16_t>(kGzMarker | static_cast<uint16_t>((kGzWindow + at) & (kGzWindow - 1)));
                }
            }
            opos += len;
        }
        if (err != kInfOk) break;
        if (br.bit_pos() > end_bit) { err = kInfInput; break; }                // the block's end lies behind the buffer
    }
    // A refusal raised where the reader was within 64 bits of the buffer's end may come from the zeros behind it (a block header that
    // straddles the end of the span fails as a bad code): it says "more input", and the host decides what that means.
    if (err != kInfOk && br.bit_pos() + 64 > end_bit) err = kInfInput;
    if (kWrite && err == kInfOk && opos != c.out_len) err = kInfSize;
    return GzResult{opos, br.bit_pos(), fin ? 1 : 0, err, reach};
}

__global__ __launch_bounds__(64) void gz_size_kernel(const uint32_t *in, int64_t n_bytes, const GzChunk *chunks, GzResult *res, int64_t n)
{
    __shared__ CodeTables t;
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const GzResult r = inflate_chunk<false>(in, n_bytes, chunks[i], nullptr, t);
    if ((threadIdx.x & 63) == 0) res[i] = r;
}

__global__ __launch_bounds__(64) void gz_decode_kernel(const uint32_t *in, int64_t n_bytes, const GzChunk *chunks, GzResult *res, int64_t n, uint16_t *sym)
{
    __shared__ CodeTables t;
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const GzChunk c = chunks[i];
    const GzResult r = inflate_chunk<true>(in, n_bytes, c, sym + c.out_off, t);
    if ((threadIdx.x & 63) == 0) res[i] = r;
}

// 64 bits of the buffer from bit `bit` on (zeros beyond the buffer)
__device__ __forceinline__ uint64_t gz_bits64(const uint32_t *in, int64_t last, int64_t bit)
{
    const int64_t j = bit >> 5;
    const int sh = static_cast<int>(bit & 31);
    auto ld = [&](int64_t k) { return (k >= 0 && k <= last) ? in[k] : 0u; };
    uint64_t v = (static_cast<uint64_t>(ld(j)) | (static_cast<uint64_t>(ld(j + 1)) << 32)) >> sh;
    if (sh) v |= static_cast<uint64_t>(ld(j + 2)) << (64 - sh);
    return v;
}

// hit[c]: the first bit in [(c + 1) * stride * 8, (c + 2) * stride * 8) at which a non-final dynamic block header parses completely; -1: none
__global__ __launch_bounds__(64) void gz_find_kernel(const uint32_t *in, int64_t n_bytes, int64_t stride, int64_t n_cuts, int64_t *hit)
{
    __shared__ CodeTables t;
    const int lane = threadIdx.x & 63;
    const int64_t c = blockIdx.x;
    if (c >= n_cuts) return;
    const Code lit{t.lit_primary, t.lit_sorted, t.lit_count, kLitBits}, dist{t.dist_primary, t.dist_sorted, t.dist_count, kDistBits},
               pre{t.pre_primary, t.pre_sorted, t.pre_count, 7};
    const int64_t end_bit = n_bytes * 8, last = n_bytes > 0 ? (n_bytes - 1) >> 2 : -1;
    const int64_t lo = (c + 1) * stride * 8, hi = (c + 2) * stride * 8 < end_bit ? (c + 2) * stride * 8 : end_bit;
    int64_t found = -1;
    for (int64_t p0 = lo; p0 < hi && found < 0; p0 += 64) {
        const int64_t p = p0 + lane;
        const uint64_t h = gz_bits64(in, last, p);                             // BFINAL, BTYPE, HLIT, HDIST, HCLEN: 17 bits
        const uint32_t hclen = (static_cast<uint32_t>(h >> 13) & 15u) + 4;
        bool ok = p < hi && (h & 7u) == 4u && ((h >> 3) & 31u) <= 29u && ((h >> 8) & 31u) <= 29u && p + 17 + 3 * hclen <= end_bit;
        if (ok) {                                                              // the code-length code is complete (zlib refuses any other)
            const uint64_t pc = gz_bits64(in, last, p + 17);
            uint32_t kraft = 0;
#pragma unroll
            for (uint32_t i = 0; i < 19; i++) {
                const uint32_t v = i < hclen ? static_cast<uint32_t>(pc >> (3 * i)) & 7u : 0u;
                kraft += v ? 128u >> v : 0u;
            }
            ok = kraft == 128u;
        }
        unsigned long long m = __ballot(ok);
        while (m && found < 0) {                                               // (uniform) the survivors, in order, by the whole wave
            const int b = __ffsll(static_cast<long long>(m)) - 1;
            m &= m - 1;
            const int64_t q = p0 + b;
            BitReader br;
            br.base = in;
            br.last = last;
            br.seek(q);
            br.refill();
            br.drop(3);
            if (read_block_codes(2, br, t.lens, pre, lit, dist) == kInfOk && br.bit_pos() <= end_bit) found = q;
        }
    }
    if (lane == 0) hit[c] = found;
}

// The starting window of every chunk, in order: win[i] = the 32 KiB of text before chunk i.  One workgroup, the running window in LDS.
// carry: the window before chunk 0 (in), behind the last chunk (out).
__global__ __launch_bounds__(1024) void gz_chain_kernel(const uint16_t *sym, const GzChunk *chunks, int64_t n, uint8_t *win, uint8_t *carry)
{
    __shared__ uint8_t w[2][kGzWindow];
    const int tid = threadIdx.x;
    for (int j = tid; j < kGzWindow; j += 1024) w[0][j] = carry[j];
    __syncthreads();
    int cur = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t L = chunks[i].out_len;
        const uint16_t *s = sym + chunks[i].out_off;
        uint8_t *wi = win + i * kGzWindow;
        for (int j = tid; j < kGzWindow; j += 1024) {
            const uint8_t old = w[cur][j];
            wi[j] = old;
            const int64_t p = L - kGzWindow + j;                              // the chunk's symbol that ends up at window index j
            uint8_t b;
            if (p >= 0) {
                const uint16_t v = s[p];
                b = v < 256 ? static_cast<uint8_t>(v) : w[cur][v & (kGzWindow - 1)];
            } else {
                b = w[cur][(j + L) & (kGzWindow - 1)];                         // a chunk shorter than the window: the old one moves up
            }
            w[cur ^ 1][j] = b;
        }
        __syncthreads();
        cur ^= 1;
    }
    for (int j = tid; j < kGzWindow; j += 1024) carry[j] = w[cur][j];
}

// text[g] = the byte of symbol g; a reference reads the window of the chunk g lies in.  off[0 .. n] ascend, off[n] = total.
__global__ __launch_bounds__(256) void gz_resolve_kernel(const uint16_t *sym, const GzChunk *chunks, int64_t n, int64_t total, const uint8_t *win,
                                                         uint8_t *text, int32_t *bad)
{
    const int64_t g0 = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 8;
    if (g0 >= total) return;
    int64_t lo = 0, hi = n - 1;                                               // the last chunk that starts at or before g0
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (chunks[mid].out_off <= g0) lo = mid; else hi = mid - 1;
    }
    int64_t c = lo;
    const int cnt = total - g0 < 8 ? static_cast<int>(total - g0) : 8;
    uint16_t v[8];
    if (cnt == 8) {
        const uint4 q = *reinterpret_cast<const uint4 *>(sym + g0);
        v[0] = q.x & 0xffff; v[1] = q.x >> 16; v[2] = q.y & 0xffff; v[3] = q.y >> 16;
        v[4] = q.z & 0xffff; v[5] = q.z >> 16; v[6] = q.w & 0xffff; v[7] = q.w >> 16;
    } else {
        for (int k = 0; k < 8; k++) v[k] = k < cnt ? sym[g0 + k] : 0;
    }
    uint8_t out[8];
    bool marker_in_first = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        while (c + 1 < n && chunks[c + 1].out_off <= g0 + k) c++;
        uint8_t b = static_cast<uint8_t>(v[k]);
        if (v[k] >= 256 && k < cnt) {
            b = win[c * kGzWindow + (v[k] & (kGzWindow - 1))];
            if (chunks[c].first) marker_in_first = true;
        }
        out[k] = b;
    }
    if (cnt == 8) {
        uint2 o;
        o.x = out[0] | (out[1] << 8) | (out[2] << 16) | (static_cast<uint32_t>(out[3]) << 24);
        o.y = out[4] | (out[5] << 8) | (out[6] << 16) | (static_cast<uint32_t>(out[7]) << 24);
        *reinterpret_cast<uint2 *>(text + g0) = o;
    } else {
        for (int k = 0; k < cnt; k++) text[g0 + k] = out[k];
    }
    if (marker_in_first) atomicOr(bad, 1);
}

namespace {

struct DevMem {                                                                // grow-only device buffer
    void *p = nullptr;
    size_t bytes = 0;
    ~DevMem() { if (p) (void)hipFree(p); }
    hipError_t need(size_t n)
    {
        if (n <= bytes) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; bytes = 0; }
        const hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct Lap {                                                                   // wall time of a stage that ends waited for
    double &acc;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    explicit Lap(double &a) : acc(a) {}
    ~Lap() { acc += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_gzip_inflate(palace_ctx *ctx, const uint8_t *file, int64_t size, const palace_gzip_params *prm, palace_gzip_sink sink,
                                   void *user, palace_gzip_stats *st)
{
    PALACE_REQUIRE(ctx && file && size >= 0 && sink && st, "bad argument");
    std::memset(st, 0, sizeof *st);
    const int64_t stride = std::max<int64_t>(16, prm && prm->stride > 0 ? prm->stride : 16 << 10);
    const int64_t span = std::max<int64_t>(64, prm && prm->span > 0 ? prm->span : 64ll << 20);
    const int64_t cap = std::min<int64_t>(1ll << 30, std::max<int64_t>(1 << 16, prm && prm->text_cap > 0 ? prm->text_cap : 512ll << 20));
    PALACE_REQUIRE(span < (1ll << 40) && stride < (1ll << 40), "bad argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const bool guards = prm && prm->check_guards;
    auto decline = [&](int why) { st->fallback = why; return PALACE_OK; };

    DevMem d_in, d_sym, d_text, d_win, d_meta, d_small;
    PALACE_HIP_TRY(d_small.need(kGzWindow + 64));                              // the carried window, and the resolve kernel's flag behind it
    uint8_t *const d_carry = d_small.as<uint8_t>();
    int32_t *const d_bad = reinterpret_cast<int32_t *>(d_carry + kGzWindow);
    PALACE_HIP_TRY(hipMemsetAsync(d_carry, 0, kGzWindow + 64, s));

    const int64_t hdr = palace_host::gzip_header_end(file, static_cast<size_t>(size), 0);
    if (hdr < 0) return decline(PALACE_GZ_HEADER);
    int64_t cur_abs = hdr * 8;                                                 // the certain start: a bit of the file
    int32_t first = 1;
    int64_t member_text = 0;                                                   // of the member cur_abs lies in, before cur_abs
    bool file_done = false;
    palace_host::MemberCheck check;
    std::vector<GzChunk> ch;
    std::vector<GzResult> res;
    std::vector<int64_t> hits;
    std::vector<palace_host::GzAccepted> acc;
    std::vector<uint8_t> meta;

    // the size pass for ch[i0 .. i0 + n): results to res[i0 ..]
    auto size_pass = [&](size_t i0, size_t n, int64_t n_bytes) -> int {
        Lap lap(st->ms_size);
        PALACE_HIP_TRY(d_meta.need((ch.size() + 1) * (sizeof(GzChunk) + sizeof(GzResult))));
        GzChunk *dc = d_meta.as<GzChunk>();
        GzResult *dr = reinterpret_cast<GzResult *>(dc + n);
        PALACE_HIP_TRY(hipMemcpyAsync(dc, ch.data() + i0, n * sizeof(GzChunk), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(gz_size_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, s, d_in.as<uint32_t>(), n_bytes, dc, dr, static_cast<int64_t>(n));
        PALACE_HIP_TRY(hipGetLastError());
        PALACE_HIP_TRY(hipMemcpyAsync(res.data() + i0, dr, n * sizeof(GzResult), hipMemcpyDeviceToHost, s));
        PALACE_HIP_TRY(hipStreamSynchronize(s));
        return PALACE_OK;
    };

    while (!file_done) {
        // ---- a span of compressed bytes: [a, b) of the file ----
        const int64_t a = (cur_abs >> 3) & ~int64_t{3}, b = std::min(size, a + span), n_bytes = b - a;
        if (n_bytes <= 0) return decline(PALACE_GZ_TRUNCATED);
        const bool at_eof = b == size;
        const int64_t rel = a * 8, end_bits = n_bytes * 8, cur = cur_abs - rel;
        st->spans++;
        {
            Lap lap(st->ms_upload);
            PALACE_HIP_TRY(d_in.need(static_cast<size_t>(n_bytes) + 64));
            PALACE_HIP_TRY(hipMemcpyAsync(d_in.p, file + a, static_cast<size_t>(n_bytes), hipMemcpyHostToDevice, s));
            PALACE_HIP_TRY(hipStreamSynchronize(s));
        }
        const int64_t n_cuts = std::max<int64_t>(0, (n_bytes + stride - 1) / stride - 1);
        PALACE_REQUIRE(n_cuts < (1ll << 31), "stride too small for the span");
        hits.assign(static_cast<size_t>(n_cuts), -1);
        if (n_cuts) {
            Lap lap(st->ms_find);
            PALACE_HIP_TRY(d_meta.need(static_cast<size_t>(n_cuts) * 8));
            hipLaunchKernelGGL(gz_find_kernel, dim3(static_cast<unsigned>(n_cuts)), dim3(64), 0, s, d_in.as<uint32_t>(), n_bytes, stride, n_cuts, d_meta.as<int64_t>());
            PALACE_HIP_TRY(hipGetLastError());
            PALACE_HIP_TRY(hipMemcpyAsync(hits.data(), d_meta.p, static_cast<size_t>(n_cuts) * 8, hipMemcpyDeviceToHost, s));
            PALACE_HIP_TRY(hipStreamSynchronize(s));
        }
        ch.clear();
        ch.push_back(GzChunk{cur, end_bits, 0, 0, 0, 0});
        for (int64_t h : hits)
            if (h > cur && h < end_bits) { ch.back().stop = h; ch.push_back(GzChunk{h, end_bits, 0, 0, 0, 0}); }
        st->chunks_found += static_cast<int64_t>(ch.size()) - 1;
        res.assign(ch.size() + 1, GzResult{0, 0, 0, 0, 0});
        if (int rc = size_pass(0, ch.size(), n_bytes)) return rc;

        // ---- the chain (host/gzip_member.hpp) ----
        const palace_host::GzSpan sp{file, size, a, end_bits, at_eof, cap, kGzMaxRounds};
        palace_host::GzChainState cs{cur, first, false, member_text};
        const std::vector<GzChunk> cand = ch;
        const std::vector<GzResult> cand_res(res.begin(), res.begin() + static_cast<long>(cand.size()));
        int device_rc = 0;
        const int why = palace_host::gz_chain_walk(sp, cand, cand_res, cs, acc, [&](const GzChunk &c, GzResult *r) -> int {
            ch.assign(1, c);
            res.assign(2, GzResult{0, 0, 0, 0, 0});
            if (int rc = size_pass(0, 1, n_bytes)) return rc;
            *r = res[0];
            return 0;
        }, &device_rc);
        st->false_hits += cs.false_hits; st->rounds += cs.rounds; st->members += cs.members;
        if (why < 0) return device_rc;
        if (why) return decline(why);
        first = cs.first; file_done = cs.file_done; member_text = cs.member_text;
        cur_abs = rel + cs.pos;
        st->chunks_accepted += static_cast<int64_t>(acc.size());

        // ---- the chain's chunks to text, a batch of at most `cap` bytes at a time ----
        for (size_t j0 = 0; j0 < acc.size();) {
            size_t j1 = j0;
            int64_t total = 0;
            while (j1 < acc.size() && static_cast<int64_t>(j1 - j0) < kGzMaxBatchChunks && (j1 == j0 || total + acc[j1].out_len <= cap)) total += acc[j1++].out_len;
            const size_t n = j1 - j0;
            st->batches++;
            // device tables: chunks, results, and the ranges palace_crc32_members takes
            const size_t o_res = n * sizeof(GzChunk), o_off = o_res + n * sizeof(GzResult), o_len = o_off + n * 8, o_crc = o_len + n * 4, m_bytes = o_crc + n * 4;
            meta.assign(m_bytes, 0);
            GzChunk *hc = reinterpret_cast<GzChunk *>(meta.data());
            int64_t *h_off = reinterpret_cast<int64_t *>(meta.data() + o_off);
            int32_t *h_len = reinterpret_cast<int32_t *>(meta.data() + o_len);
            int64_t off = 0;
            for (size_t k = 0; k < n; k++) {
                const palace_host::GzAccepted &ac = acc[j0 + k];
                hc[k] = GzChunk{ac.start, ac.end, off, ac.out_len, ac.first, 0};
                h_off[k] = off; h_len[k] = static_cast<int32_t>(ac.out_len);
                off += ac.out_len;
            }
            PALACE_HIP_TRY(d_meta.need(m_bytes + 64));
            // every output buffer lies between two 64-byte guards (prm->check_guards: filled before, looked at after the batch)
            const size_t used[3] = {static_cast<size_t>(total) * 2, static_cast<size_t>(total), n * kGzWindow};
            DevMem *const outs[3] = {&d_sym, &d_text, &d_win};
            for (int q = 0; q < 3; q++) {
                PALACE_HIP_TRY(outs[q]->need(used[q] + 192));
                if (!guards) continue;
                PALACE_HIP_TRY(hipMemsetAsync(outs[q]->p, 0xa5, 64, s));
                PALACE_HIP_TRY(hipMemsetAsync(outs[q]->as<uint8_t>() + 64 + used[q], 0xa5, 64, s));
            }
            auto look_at_guards = [&]() -> int {
                if (!guards) return PALACE_OK;
                uint8_t g[3][128];
                for (int q = 0; q < 3; q++) {
                    PALACE_HIP_TRY(hipMemcpyAsync(g[q], outs[q]->p, 64, hipMemcpyDeviceToHost, s));
                    PALACE_HIP_TRY(hipMemcpyAsync(g[q] + 64, outs[q]->as<uint8_t>() + 64 + used[q], 64, hipMemcpyDeviceToHost, s));
                }
                PALACE_HIP_TRY(hipStreamSynchronize(s));
                for (int q = 0; q < 3; q++)
                    for (int k = 0; k < 128; k++)
                        if (g[q][k] != 0xa5) st->guards_bad++;
                return PALACE_OK;
            };
            uint16_t *const b_sym = reinterpret_cast<uint16_t *>(d_sym.as<uint8_t>() + 64);
            uint8_t *const b_text = d_text.as<uint8_t>() + 64, *const b_win = d_win.as<uint8_t>() + 64;
            uint8_t *dm = d_meta.as<uint8_t>();
            GzChunk *dc = reinterpret_cast<GzChunk *>(dm);
            GzResult *dr = reinterpret_cast<GzResult *>(dm + o_res);
            res.assign(n + 1, GzResult{0, 0, 0, 0, 0});
            {
                Lap lap(st->ms_decode);
                PALACE_HIP_TRY(hipMemcpyAsync(dm, meta.data(), o_crc, hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(gz_decode_kernel, dim3(static_cast<unsigned>(n)), dim3(64), 0, s, d_in.as<uint32_t>(), n_bytes, dc, dr, static_cast<int64_t>(n), b_sym);
                PALACE_HIP_TRY(hipGetLastError());
                PALACE_HIP_TRY(hipMemcpyAsync(res.data(), dr, n * sizeof(GzResult), hipMemcpyDeviceToHost, s));
                PALACE_HIP_TRY(hipStreamSynchronize(s));
            }
            for (size_t k = 0; k < n; k++)
                if (res[k].status != kInfOk || res[k].end_bit != acc[j0 + k].end || res[k].out_len != acc[j0 + k].out_len) {
                    if (int rc = look_at_guards()) return rc;                 // (the one kernel whose writes follow the input)
                    return decline(PALACE_GZ_DECODE);
                }
            {
                Lap lap(st->ms_chain);
                hipLaunchKernelGGL(gz_chain_kernel, dim3(1), dim3(1024), 0, s, b_sym, dc, static_cast<int64_t>(n), b_win, d_carry);
                PALACE_HIP_TRY(hipGetLastError());
                PALACE_HIP_TRY(hipStreamSynchronize(s));
            }
            std::vector<uint32_t> crc(n);
            int32_t bad = 0;
            if (total) {
                Lap lap(st->ms_resolve);
                const int64_t groups = (total + 7) / 8;
                hipLaunchKernelGGL(gz_resolve_kernel, dim3(static_cast<unsigned>((groups + 255) / 256)), dim3(256), 0, s, b_sym, dc, static_cast<int64_t>(n), total,
                                   b_win, b_text, d_bad);
                PALACE_HIP_TRY(hipGetLastError());
                PALACE_HIP_TRY(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, s));
                PALACE_HIP_TRY(hipStreamSynchronize(s));
            }
            if (int rc = look_at_guards()) return rc;
            if (bad) return decline(PALACE_GZ_MARKER);
            {
                Lap lap(st->ms_crc);
                if (int rc = palace_crc32_members(ctx, b_text, static_cast<int64_t>(n), reinterpret_cast<const int64_t *>(dm + o_off),
                                                  reinterpret_cast<const int32_t *>(dm + o_len), reinterpret_cast<uint32_t *>(dm + o_crc))) return rc;
                PALACE_HIP_TRY(hipMemcpyAsync(crc.data(), dm + o_crc, n * 4, hipMemcpyDeviceToHost, s));
                PALACE_HIP_TRY(hipStreamSynchronize(s));
                for (size_t k = 0; k < n; k++) {
                    check.add(crc[k], acc[j0 + k].out_len);
                    if (acc[j0 + k].trailer < 0) continue;
                    const int v = check.verdict(file + acc[j0 + k].trailer);
                    if (v) return decline(v == 1 ? PALACE_GZ_CRC : PALACE_GZ_ISIZE);
                    check.reset();
                }
            }
            const bool last = file_done && j1 == acc.size();
            if (total || last) {
                Lap lap(st->ms_sink);
                if (sink(user, b_text, total, last ? 1 : 0)) return decline(PALACE_GZ_SINK);
            }
            st->text_bytes += total;
            j0 = j1;
        }
    }
    return PALACE_OK;
}
