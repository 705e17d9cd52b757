// N4 on the device: the BGZF members of a BAM file inflated by the GPU, one wavefront per member.
//
// A BGZF member is an independent raw DEFLATE stream (RFC 1951) of at most 64 KiB of output; a 0.9 GB BAM holds ~36 000 of
// them.  DEFLATE decoding is serial inside a stream -- a symbol's position in the bit stream is known only when the one
// before it is decoded -- so the parallelism is across members: every member gets a wavefront whose 64 lanes all run the SAME
// decode (no divergence, nothing to broadcast) and split what is parallel inside a member: building the code tables,
// copying matches.  DEFLATE's window (the last 32 KiB of output) is the output buffer itself: a match reads the bytes it repeats
// back from where the wave wrote them (L2), which costs a wave a round trip per match -- and leaves a wave 4 KiB of LDS (its code
// tables) instead of 36, so that a CU holds 32 of them instead of 4.  The decode of ONE stream is a chain of dependent steps that
// issues an instruction every ~10 cycles; with one wave per SIMD (window in LDS: the first version, 5.7 GB/s of output for a
// whole BAM) the chip idled behind those latencies, with eight they overlap.
//
// Input words reach the lanes through a register window: lane l holds dword (base + l) of the member, the decode takes dword
// j with one v_readlane, and the following 64 dwords are always already requested -- the bit reader never waits for HBM.
//
// Memory safety does not depend on the input: input dwords are fetched only inside [first, last] dword of the member (zeros
// beyond), every LDS index is masked, every write to the output is bounded by the member's out_len, and every loop consumes
// input or produces output, both of which are bounded.  A member the decoder refuses (malformed, or a size mismatch) gets a
// non-zero status and the host decides it with zlib, which stays the authority on malformed input (as for the CPU decoder,
// host/inflate_fast.hpp).
#include "common.hpp"
#include "deflate.hpp"

namespace palace {

struct InflateArgs {
    const uint8_t *in;
    const int64_t *in_off;
    const int32_t *in_len;
    const int64_t *out_off;
    const int32_t *out_len;
    uint8_t *out;
    int32_t *status;
    int64_t n_members;
};

__global__ __launch_bounds__(64) void bgzf_inflate_kernel(InflateArgs a)
{
    __shared__ uint16_t lit_primary[1 << kLitBits], lit_sorted[288], lit_count[16];
    __shared__ uint16_t dist_primary[1 << kDistBits], dist_sorted[32], dist_count[16];
    __shared__ uint16_t pre_primary[1 << 7], pre_sorted[19], pre_count[16];
    __shared__ uint8_t lens[352];                                            // [0, 19) code-length code; [20, 20 + 316) the block's lengths
    const int lane = threadIdx.x & 63;
    const int64_t m = blockIdx.x;
    if (m >= a.n_members) return;
    const int64_t in_off = a.in_off[m], out_off = a.out_off[m];
    const int32_t in_len = a.in_len[m], out_len = a.out_len[m];
    if (in_len < 0 || out_len < 0 || out_len > 65536 + 0) { if (lane == 0) a.status[m] = kInfSize; return; }
    if (out_len == 0 && in_len == 0) { if (lane == 0) a.status[m] = kInfOk; return; }
    const Code lit{lit_primary, lit_sorted, lit_count, kLitBits}, dist{dist_primary, dist_sorted, dist_count, kDistBits},
               pre{pre_primary, pre_sorted, pre_count, 7};
    BitReader br;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(a.in + in_off);
    br.base = reinterpret_cast<const uint32_t *>(addr & ~static_cast<uintptr_t>(3));
    const int skip = static_cast<int>(addr & 3);
    br.last = in_len > 0 ? (skip + static_cast<int64_t>(in_len) - 1) >> 2 : -1;
    br.seek(skip * 8);
    const int64_t end_bit = (skip + static_cast<int64_t>(in_len)) * 8;     // the member's DEFLATE data ends here
    uint8_t *const out = a.out + out_off;
    int32_t opos = 0, err = kInfOk;
    // what the wave wrote so far is in memory before anything reads it back (a match's source may be a literal lane 0 stored a moment
    // ago): a release fence of the wave's stores, then loads that are served where the stores went
    auto written = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); };
    auto back = [&](int32_t at) { return __hip_atomic_load(out + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    bool last_block = false;
    while (!last_block && err == kInfOk) {
        br.refill();
        last_block = br.take(1) != 0;
        const uint32_t btype = br.take(2);
        if (btype == 0) {
            // stored: LEN / NLEN at the next byte boundary, then LEN raw bytes
            const int64_t p_bit = (br.bit_pos() + 7) & ~7ll;
            br.seek(p_bit);
            br.refill();
            const uint32_t len = br.take(16);
            br.refill();
            const uint32_t nlen = br.take(16);
            if ((len ^ 0xffffu) != nlen) { err = kInfBadBlock; break; }
            const int64_t data_bit = p_bit + 32;
            if (data_bit + static_cast<int64_t>(len) * 8 > end_bit || static_cast<int32_t>(len) > out_len - opos) { err = kInfOverrun; break; }
            const uint8_t *src = reinterpret_cast<const uint8_t *>(br.base) + (data_bit >> 3);
            for (uint32_t i = lane; i < len; i += 64) out[opos + static_cast<int32_t>(i)] = src[i];
            opos += static_cast<int32_t>(len);
            br.seek(data_bit + static_cast<int64_t>(len) * 8);
            continue;
        }
        if (btype == 3) { err = kInfBadBlock; break; }
        err = read_block_codes(btype, br, lens, pre, lit, dist);
        if (err != kInfOk) break;
        // ---- the block's symbols ----
        for (;;) {
            br.refill();                                                       // >= 33 bits: a literal/length code and its extra bits
            if (br.bit_pos() > end_bit + 64) { err = kInfInput; break; }       // far past the member's data: a stream that does not end
            const int sym = decode_sym(lit, br);
            if (sym < 0) { err = kInfBadCode; break; }
            if (sym < 256) {
                if (opos >= out_len) { err = kInfOverrun; break; }
                if (lane == 0) out[opos] = static_cast<uint8_t>(sym);
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
            br.refill();                                                       // (a distance code may have used 15 of the 33 bits)
            dist_code(ds, dbase, dextra);
            const int32_t d = dbase + static_cast<int32_t>(br.take(dextra));
            if (d > opos) { err = kInfBadDistance; break; }
            if (len > out_len - opos) { err = kInfOverrun; break; }
            // the copy: sources lie below opos, destinations at and above it; an overlapping match (d < len) repeats its d bytes
            written();
            for (int32_t i = lane; i < len; i += 64) {
                const int32_t s = d >= len ? i : i % d;
                out[opos + i] = back(opos - d + s);
            }
            opos += len;
        }
    }
    if (err == kInfOk) {
        if (opos != out_len) err = kInfSize;
        else if (br.bit_pos() > end_bit + 7) err = kInfInput;                  // the stream ran past the member's data
    }
    if (lane == 0) a.status[m] = err;
}

}  // namespace palace

using namespace palace;

extern "C" int palace_bgzf_inflate(palace_ctx *ctx, const uint8_t *d_in, int64_t n_members, const int64_t *d_in_off, const int32_t *d_in_len,
                                   const int64_t *d_out_off, const int32_t *d_out_len, uint8_t *d_out, int32_t *d_status)
{
    PALACE_REQUIRE(ctx && n_members >= 0 && n_members < (1ll << 31), "bad argument");
    if (n_members == 0) return PALACE_OK;
    PALACE_REQUIRE(d_in && d_in_off && d_in_len && d_out_off && d_out_len && d_out && d_status, "null device pointer");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const InflateArgs a{d_in, d_in_off, d_in_len, d_out_off, d_out_len, d_out, d_status, n_members};
    hipLaunchKernelGGL(bgzf_inflate_kernel, dim3(static_cast<unsigned>(n_members)), dim3(64), 0, ctx->stream, a);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
