// What the kernels that read a text 16 bytes a lane share (fastq.hip, depth_parse.hip, sam.hip, the FASTA index of path_fasta.hip,
// the checks of fastg_split.hip): a lane's 16 bytes of a text window, the mask of its newlines, and the
// workgroup's exclusive prefix sum that turns newline counts into line ordinals -- which is also the block step of every scan of
// scan64.hpp.  The lanes that WRITE a text are window_lanes.hpp's.
#pragma once
#include "common.hpp"

namespace palace {

constexpr int kLaneBytes = 16;

// the lane's 16 bytes (zeros and valid = 0 past the end of the text)
__device__ __forceinline__ int load_lane(const uint8_t *text, int64_t n, int64_t at, uint32_t w[4])
{
    if (at + kLaneBytes <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + at);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return kLaneBytes;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
    const int valid = at < n ? static_cast<int>(n - at) : 0;
    for (int k = 0; k < valid; k++) w[k >> 2] |= static_cast<uint32_t>(text[at + k]) << (8 * (k & 3));
    return valid;
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t w[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }

// mask of the lane's newline bytes (bit k = byte k)
__device__ __forceinline__ uint32_t newline_mask(const uint32_t w[4], int valid)
{
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t x = w[q] ^ 0x0a0a0a0au;                               // a zero byte where the byte was '\n'
        const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   // bit 7 of each zero byte (exact, no carries)
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4 * q);
    }
    return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

// exclusive prefix sum over the workgroup (blockDim.x = nthreads, a multiple of 64); total returned in *total
template <class T, int nthreads>
__device__ __forceinline__ T block_exclusive(T v, T *lds, T *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
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

}  // namespace palace
