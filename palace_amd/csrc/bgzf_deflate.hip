// The writing side of BGZF on the device: the counterpart of palace_bgzf_inflate (inflate.hip).  One workgroup of 512 threads per
// member; the member's text (at most 0xff00 bytes) is staged in LDS and leaves as header + one DEFLATE block + CRC-32 + ISIZE in a
// slot of 65 536 bytes.  How a member is built -- the previous-line tokens, the per-member Huffman codes, the bit string put
// together without two lanes storing to one dword -- is deflate_enc.hpp, which a CPU build runs as well.  The output is a function
// of the input alone: histograms are integer sums, the symbol order is (frequency, symbol), bit offsets come from a scan.
//
// LDS: 73 KiB per workgroup, two workgroups (16 waves) per CU.  palace_bgzf_deflate_lz writes the same member from another token source
// (deflate_lz.hpp: hashed matches for text without lines, a BAM's): 137 KiB of LDS, one workgroup per CU.  palace_bgzf_compact moves the members of a batch next to each other
// (an exclusive scan of their lengths), so that a batch crosses PCIe as one copy of the file's bytes.
#include "common.hpp"
#include "deflate_enc.hpp"
#include "deflate_lz.hpp"

namespace palace {
namespace {

static_assert(sizeof(EncShared) <= 80 * 1024, "two workgroups per CU need at most 80 KiB of LDS each");

// The member of the text in s (n / mis / chunk / crc set, the tables cleared, all of it visible to the workgroup) into its slot, with
// the tokens of `walk`: the phases of deflate_enc.hpp, the segment scan done by the workgroup.
template <class W>
__device__ __forceinline__ void encode_member(EncShared &s, uint32_t *wave_sum, int tid, uint32_t *slot, const W &walk)
{
    enc_phase_freq(s, tid, walk);
    __syncthreads();
    enc_phase_sort(s, tid);
    __syncthreads();
    enc_phase_codes(s, tid);
    __syncthreads();
    enc_phase_cl_freq(s, tid);
    __syncthreads();
    enc_phase_cl_code(s, tid);
    __syncthreads();
    // segment lengths -> offsets: segment 0 (header) is set, segment 1 + tid is this thread's; thread 0 carries the header's bits too
    {
        const uint32_t mine = enc_token_bits(s, tid, walk), head = s.seg_off[0];
        uint32_t x = mine + (tid == 0 ? head : 0);
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if ((tid & 63) >= d) x += y;
        }
        if ((tid & 63) == 63) wave_sum[tid >> 6] = x;
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < (tid >> 6); w++) before += wave_sum[w];
        const uint32_t incl = before + x;                                  // bits of segments 0 .. 1 + tid
        s.seg_off[1 + tid] = incl - mine;
        if (tid == 0) s.seg_off[0] = 0;
        if (tid == kEncThreads - 1) enc_finish_scan(s, incl);
    }
    __syncthreads();
    enc_phase_write(s, tid, slot, walk);
    __syncthreads();
    enc_phase_merge(s, tid, slot);
}

__global__ __launch_bounds__(kEncThreads) void bgzf_deflate_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ off,
                                                                   const int32_t *__restrict__ len, const uint32_t *__restrict__ crc,
                                                                   uint8_t *__restrict__ slots, int32_t *__restrict__ member_len)
{
    __shared__ EncShared s;
    __shared__ uint32_t wave_sum[kEncThreads / 64];
    const int tid = threadIdx.x;
    const int64_t m = blockIdx.x;
    uint32_t *slot = reinterpret_cast<uint32_t *>(slots + m * kEncSlot);
    int32_t n = len[m];
    n = n < 0 ? 0 : n > kEncMaxText ? kEncMaxText : n;                     // (the entry point documents the range; nothing is read or written outside it)
    if (n == 0) {
        enc_write_empty(tid, slot);
        if (tid == 0) member_len[m] = 28;
        return;
    }
    // whole dwords of the source, so that the text keeps its misalignment in LDS (an aligned dword never crosses a page)
    const uintptr_t addr = reinterpret_cast<uintptr_t>(text + off[m]);
    const int mis = static_cast<int>(addr & 3);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(addr - mis);
    for (int i = tid; i < (mis + n + 3) / 4; i += kEncThreads) s.text[i] = src[i];
    if (tid == 0) {
        s.n = n; s.mis = mis; s.chunk = (n + kEncThreads - 1) / kEncThreads; s.crc = crc[m];
    }
    enc_phase_clear(s, tid);
    __syncthreads();
    encode_member(s, wave_sum, tid, slot, EncLineWalk{});
    if (tid == 0) member_len[m] = static_cast<int32_t>(s.member_len);
}

static_assert(sizeof(LzShared) + 64 <= 160 * 1024, "the text, the tables and the head table are one workgroup's LDS: one workgroup per CU");

// The same member from the tokens of deflate_lz.hpp.  A workgroup takes members blockIdx.x, + gridDim.x, ... (the grid is at most one
// workgroup per CU, which is all that LDS admits) and keeps the distances of the member at hand in its own kLzDistBytes of dist_all.
__global__ __launch_bounds__(kEncThreads) void bgzf_deflate_lz_kernel(const uint8_t *__restrict__ text, const int64_t *__restrict__ off,
                                                                      const int32_t *__restrict__ len, const uint32_t *__restrict__ crc,
                                                                      uint8_t *__restrict__ slots, int32_t *__restrict__ member_len, int64_t n_members,
                                                                      uint16_t *dist_all)
{
    __shared__ LzShared s;
    __shared__ uint32_t wave_sum[kEncThreads / 64];
    const int tid = threadIdx.x;
    uint16_t *dist = dist_all + blockIdx.x * (kLzDistBytes / 2);
    for (int64_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        uint32_t *slot = reinterpret_cast<uint32_t *>(slots + m * kEncSlot);
        int32_t n = len[m];
        n = n < 0 ? 0 : n > kEncMaxText ? kEncMaxText : n;
        if (n == 0) {                                                      // (the same for every thread; LDS is not touched)
            enc_write_empty(tid, slot);
            if (tid == 0) member_len[m] = 28;
            continue;
        }
        const uintptr_t addr = reinterpret_cast<uintptr_t>(text + off[m]);
        const int mis = static_cast<int>(addr & 3);
        const uint32_t *src = reinterpret_cast<const uint32_t *>(addr - mis);
        for (int i = tid; i < (mis + n + 3) / 4; i += kEncThreads) s.e.text[i] = src[i];
        if (tid == 0) {
            s.e.n = n; s.e.mis = mis; s.e.chunk = (n + kEncThreads - 1) / kEncThreads; s.e.crc = crc[m];
        }
        enc_phase_clear(s.e, tid);
        lz_phase_clear(s, tid);
        __syncthreads();
        for (int r = 0; r * kEncThreads < n; r++) {                        // dist[p], p < n, a round at a time
            lz_phase_look(s, tid, r, dist);
            __syncthreads();
            lz_phase_enter(s, tid, r);
            __syncthreads();
        }
        encode_member(s.e, wave_sum, tid, slot, LzWalk{dist});
        if (tid == 0) member_len[m] = static_cast<int32_t>(s.e.member_len);
        __syncthreads();                                                   // the next member's text and tables replace this one's
    }
}

// member offsets in the file: exclusive scan of the lengths, one workgroup (a batch has thousands of members)
__global__ __launch_bounds__(1024) void member_scan_kernel(const int32_t *__restrict__ member_len, int64_t n, int64_t *__restrict__ member_off)
{
    __shared__ int64_t wave_sum[16];
    __shared__ int64_t carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const int64_t v = i < n ? member_len[i] : 0;
        int64_t x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t y = __shfl_up(x, d, 64);
            if ((tid & 63) >= d) x += y;
        }
        if ((tid & 63) == 63) wave_sum[tid >> 6] = x;
        __syncthreads();
        int64_t before = carry;
        for (int w = 0; w < (tid >> 6); w++) before += wave_sum[w];
        if (i < n) member_off[i] = before + x - v;
        __syncthreads();
        if (tid == 1023) carry = before + x;
        __syncthreads();
    }
    if (tid == 0) member_off[n] = carry;
}

// member m's bytes from its slot to file[member_off[m] ..): whole dwords of the destination, put together from two of the slot's
__global__ __launch_bounds__(256) void member_copy_kernel(const uint8_t *__restrict__ slots, const int32_t *__restrict__ member_len,
                                                          const int64_t *__restrict__ member_off, uint8_t *__restrict__ file)
{
    const int64_t m = blockIdx.x;
    const int64_t len = member_len[m];
    const uint32_t *src = reinterpret_cast<const uint32_t *>(slots + m * kEncSlot);
    const uintptr_t dst0 = reinterpret_cast<uintptr_t>(file + member_off[m]);
    const int lead = static_cast<int>((4 - (dst0 & 3)) & 3);              // bytes in front of the first aligned dword of the destination
    uint8_t *dst = reinterpret_cast<uint8_t *>(dst0);
    const uint8_t *srcb = reinterpret_cast<const uint8_t *>(src);
    if (threadIdx.x < lead && threadIdx.x < len) dst[threadIdx.x] = srcb[threadIdx.x];
    if (len <= lead) return;
    const int64_t n_dw = (len - lead) / 4;
    uint32_t *dstw = reinterpret_cast<uint32_t *>(dst + lead);
    const int sh = lead * 8;                                               // destination dword j = source bytes [lead + 4 j, lead + 4 j + 4)
    for (int64_t j = threadIdx.x; j < n_dw; j += blockDim.x) {
        const uint32_t lo = src[j];
        const uint32_t hi = sh ? src[j + 1] : 0;                           // (j + 1 < 16 384: lead + 4 j + 4 <= len <= 65 536 and lead > 0)
        dstw[j] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    const int64_t tail = lead + n_dw * 4;
    if (tail + threadIdx.x < len) dst[tail + threadIdx.x] = srcb[tail + threadIdx.x];
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" int palace_bgzf_deflate(palace_ctx *ctx, const uint8_t *d_text, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                                   const uint32_t *d_crc, uint8_t *d_slots, int32_t *d_member_len)
{
    PALACE_REQUIRE(ctx && n_members >= 0 && n_members < (1ll << 31), "bad argument");
    if (n_members == 0) return PALACE_OK;
    PALACE_REQUIRE(d_text && d_off && d_len && d_crc && d_slots && d_member_len, "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_slots) & 3) == 0, "the slots must be 4-byte aligned");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(static_cast<unsigned>(n_members)), dim3(kEncThreads), 0, ctx->stream, d_text, d_off, d_len,
                       d_crc, d_slots, d_member_len);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bgzf_deflate_lz(palace_ctx *ctx, const uint8_t *d_text, int64_t n_members, const int64_t *d_off, const int32_t *d_len,
                                      const uint32_t *d_crc, uint8_t *d_slots, int32_t *d_member_len)
{
    PALACE_REQUIRE(ctx && n_members >= 0 && n_members < (1ll << 31), "bad argument");
    if (n_members == 0) return PALACE_OK;
    PALACE_REQUIRE(d_text && d_off && d_len && d_crc && d_slots && d_member_len, "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_slots) & 3) == 0, "the slots must be 4-byte aligned");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const int64_t grid = n_members < kCUs ? n_members : kCUs;
    const int rc = ensure_workspace(ctx, static_cast<size_t>(grid) * kLzDistBytes);
    if (rc) return rc;
    hipLaunchKernelGGL(bgzf_deflate_lz_kernel, dim3(static_cast<unsigned>(grid)), dim3(kEncThreads), 0, ctx->stream, d_text, d_off, d_len, d_crc,
                       d_slots, d_member_len, n_members, static_cast<uint16_t *>(ctx->ws.ptr));
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

extern "C" int palace_bgzf_compact(palace_ctx *ctx, const uint8_t *d_slots, int64_t n_members, const int32_t *d_member_len,
                                   uint8_t *d_file, int64_t *d_member_off)
{
    PALACE_REQUIRE(ctx && n_members >= 0 && n_members < (1ll << 31), "bad argument");
    PALACE_REQUIRE(d_member_off, "null device pointer");
    PALACE_REQUIRE(n_members == 0 || (d_slots && d_member_len && d_file), "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_slots) & 3) == 0, "the slots must be 4-byte aligned");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(member_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, d_member_len, n_members, d_member_off);
    if (n_members)
        hipLaunchKernelGGL(member_copy_kernel, dim3(static_cast<unsigned>(n_members)), dim3(256), 0, ctx->stream, d_slots, d_member_len,
                           d_member_off, d_file);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
