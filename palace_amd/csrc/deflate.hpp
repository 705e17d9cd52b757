// RFC 1951 on a wavefront: the bit reader, the canonical Huffman tables in LDS and a block header's codes, shared by the BGZF
// kernel (inflate.hip: one wavefront per member) and the gzip kernels (gzip.hip: many wavefronts inside one stream).
#pragma once
#include "common.hpp"

namespace palace {

constexpr int kLitBits = 10, kDistBits = 8;

// base value and number of extra bits of a length code (257 .. 285 -> c = 0 .. 28) and of a distance code (0 .. 29), RFC 1951 3.2.5,
// as arithmetic (a table in memory is a dependent load per symbol)
__device__ __forceinline__ void len_code(int c, int32_t &base, int &extra)
{
    if (c < 8) { base = 3 + c; extra = 0; }
    else if (c == 28) { base = 258; extra = 0; }
    else { extra = (c >> 2) - 1; base = 3 + ((4 + (c & 3)) << extra); }
}
__device__ __forceinline__ void dist_code(int c, int32_t &base, int &extra)
{
    if (c < 4) { base = 1 + c; extra = 0; }
    else { extra = (c >> 1) - 1; base = 1 + ((2 + (c & 1)) << extra); }
}
static __device__ const uint8_t kPreOrderD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

enum : int32_t { kInfOk = 0, kInfBadBlock = 1, kInfBadCode = 2, kInfBadDistance = 3, kInfOverrun = 4, kInfSize = 5, kInfInput = 6 };

// one canonical Huffman code in LDS: a primary table indexed by the next PRIMARY bits of the stream (entry = symbol | length << 9;
// 0 = the code is longer, or unused) and the canonical description (symbols in code order, count per length) for the rest
struct Code {
    uint16_t *primary;          // [1 << bits]
    uint16_t *sorted;           // symbols in code order
    uint16_t *count;            // [16]
    int bits;
};

struct BitReader {
    const uint32_t *base;       // 4-byte aligned start of the member's first dword
    int64_t last;               // index of the last dword that holds bytes of the member
    uint32_t win, win_next;     // lane l: dwords wbase + l and wbase + 64 + l
    int64_t wbase, next;        // next: index of the next dword to enter the bit buffer
    uint64_t buf;
    int cnt;

    __device__ __forceinline__ uint32_t load(int64_t j) const { return (j >= 0 && j <= last) ? base[j] : 0u; }
    __device__ __forceinline__ void seek(int64_t bit)            // position the reader at bit `bit` (from base)
    {
        const int lane = threadIdx.x & 63;
        wbase = bit >> 5;
        win = load(wbase + lane);
        win_next = load(wbase + 64 + lane);
        next = wbase;
        buf = 0; cnt = 0;
        refill();
        buf >>= (bit & 31); cnt -= static_cast<int>(bit & 31);
    }
    __device__ __forceinline__ uint32_t dword(int64_t j)         // j ascends: inside the window, or the first of the next one
    {
        if (j - wbase >= 64) {                                   // (uniform) slide: the words requested long ago become current
            win = win_next;
            wbase += 64;
            win_next = load(wbase + 64 + (threadIdx.x & 63));
        }
        return __builtin_amdgcn_readlane(win, __builtin_amdgcn_readfirstlane(static_cast<int>(j - wbase)));
    }
    __device__ __forceinline__ void refill()                     // >= 33 valid bits afterwards
    {
        if (cnt <= 32) {
            buf |= static_cast<uint64_t>(dword(next)) << cnt;
            next++;
            cnt += 32;
        }
    }
    __device__ __forceinline__ void drop(int n) { buf >>= n; cnt -= n; }
    __device__ __forceinline__ uint32_t take(int n) { const uint32_t v = static_cast<uint32_t>(buf) & ((1u << n) - 1); drop(n); return v; }
    __device__ __forceinline__ int64_t bit_pos() const { return next * 32 - cnt; }      // of the next unread bit
};

// lengths[0 .. n) -> the code's tables.  The lanes share the symbols (lane l: symbols l, l + 64, ...); a symbol's rank inside its
// length class comes from ballots, so codes are assigned in symbol order as the canonical construction demands.
// Returns false for a set zlib's inflate_table() rejects: over-subscribed, or incomplete other than a single 1-bit code
// (`lone_ok`: lengths / distances may be incomplete that way, the code-length code may not).
__device__ inline bool build_code(const Code &c, const uint8_t *lens, int n, bool lone_ok)
{
    const int lane = threadIdx.x & 63;
    for (int i = lane; i < 16; i += 64) c.count[i] = 0;
    for (int i = lane; i < (1 << c.bits); i += 64) c.primary[i] = 0;
    __builtin_amdgcn_s_waitcnt(0xc07f);                          // lgkmcnt(0): the zeros are in LDS before the adds below
    int cnt[16];
#pragma unroll
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int base = 0; base < n; base += 64) {                  // (uniform) class sizes by ballots
        const int sym = base + lane, l = sym < n ? lens[sym] : 0;
#pragma unroll
        for (int L = 1; L < 16; L++) cnt[L] += __popcll(__ballot(l == L));
    }
    int left = 1, max_len = 0, total = 0;
#pragma unroll
    for (int L = 1; L < 16; L++) {
        left = (left << 1) - cnt[L];
        if (cnt[L]) max_len = L;
        total += cnt[L];
    }
    {                                                            // over-subscribed at some length
        int lf = 1;
#pragma unroll
        for (int L = 1; L < 16; L++) { lf = (lf << 1) - cnt[L]; if (lf < 0) return false; }
    }
    if (total == 0) return lone_ok;                              // no codes: every look-up fails (allowed for lengths / distances)
    if (left > 0 && !(lone_ok && max_len == 1)) return false;    // incomplete
#pragma unroll
    for (int L = 1; L < 16; L++)
        if (lane == L) c.count[L] = static_cast<uint16_t>(cnt[L]);         // (count[0] stays 0)
    int offs[16], code0[16];                                     // first index in `sorted` / first code of every length
    offs[1] = 0; code0[1] = 0; offs[0] = 0; code0[0] = 0;
#pragma unroll
    for (int L = 1; L < 15; L++) { offs[L + 1] = offs[L] + cnt[L]; code0[L + 1] = (code0[L] + cnt[L]) << 1; }
    for (int base = 0; base < n; base += 64) {
        const int sym = base + lane, l = sym < n ? lens[sym] : 0;
        int idx = 0, code = 0;
#pragma unroll
        for (int L = 1; L < 16; L++) {
            const unsigned long long m = __ballot(l == L);
            const int before = __popcll(m & ((1ull << lane) - 1));
            if (l == L) { idx = offs[L] + before; code = code0[L] + before; }
            offs[L] += __popcll(m); code0[L] += __popcll(m);
        }
        if (l) {
            c.sorted[idx] = static_cast<uint16_t>(sym);
            if (l <= c.bits) {                                   // every primary slot whose low l bits are the reversed code
                const uint32_t rev = __brev(static_cast<uint32_t>(code)) >> (32 - l);
                const uint16_t e = static_cast<uint16_t>(sym | (l << 9));
                for (uint32_t t = rev; t < (1u << c.bits); t += 1u << l) c.primary[t] = e;
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    return true;
}

// the next symbol of code `c` (>= 0), or -1 for a bit pattern that is no code.  At least 15 bits are in the buffer.
__device__ __forceinline__ int decode_sym(const Code &c, BitReader &br)
{
    const uint32_t e = c.primary[static_cast<uint32_t>(br.buf) & ((1u << c.bits) - 1)];
    if (e) { br.drop(static_cast<int>(e >> 9)); return static_cast<int>(e & 511u); }
    // a longer code (rare): bit by bit against the canonical description
    int code = 0, first = 0, index = 0;
    uint32_t bits = static_cast<uint32_t>(br.buf);
    for (int len = 1; len <= 15; len++) {
        code |= static_cast<int>(bits & 1u);
        bits >>= 1;
        const int count = c.count[len];
        if (code - count < first) { br.drop(len); return c.sorted[index + (code - first)]; }
        index += count; first += count;
        first <<= 1; code <<= 1;
    }
    return -1;
}

// LDS of one decoding wavefront: the three codes' tables and the code lengths of the block being opened
struct CodeTables {
    uint16_t lit_primary[1 << kLitBits], lit_sorted[288], lit_count[16];
    uint16_t dist_primary[1 << kDistBits], dist_sorted[32], dist_count[16];
    uint16_t pre_primary[1 << 7], pre_sorted[19], pre_count[16];
    uint8_t lens[352];                                                       // [0, 19) code-length code; [20, 20 + 316) the block's lengths
};

// The literal/length and distance codes of a block of type 1 (fixed) or 2 (dynamic: its header is read from `br`) built into
// `lit` / `dist`; kInfOk, or why zlib would refuse the block.  (uniform: every lane runs it alike)
__device__ __forceinline__ int32_t read_block_codes(uint32_t btype, BitReader &br, uint8_t *lens, const Code &pre, const Code &lit, const Code &dist)
{
    const int lane = threadIdx.x & 63;
    if (btype == 1) {                                                          // fixed code (RFC 1951 3.2.6)
        for (int i = lane; i < 288; i += 64) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        for (int i = lane; i < 32; i += 64) lens[288 + i] = 5;
        __builtin_amdgcn_s_waitcnt(0xc07f);
        if (!build_code(lit, lens, 288, true) || !build_code(dist, lens + 288, 32, true)) return kInfBadCode;   // (32 distance codes of 5 bits: 30 and 31 never occur in valid data)
        return kInfOk;
    }
    br.refill();
    const uint32_t hlit = br.take(5) + 257, hdist = br.take(5) + 1, hclen = br.take(4) + 4;
    if (hlit > 286 || hdist > 30) return kInfBadCode;
    for (int i = lane; i < 19; i += 64) lens[i] = 0;
    __builtin_amdgcn_s_waitcnt(0xc07f);
    for (uint32_t i = 0; i < hclen; i++) {
        br.refill();
        const uint32_t v = br.take(3);
        if (lane == 0) lens[kPreOrderD[i]] = static_cast<uint8_t>(v);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (!build_code(pre, lens, 19, false)) return kInfBadCode;
    // the hlit + hdist code lengths, run-length coded with the code-length code; kept in registers of the decode (all
    // lanes alike) and stored by lane 0
    uint32_t n = 0, prev = 0;
    const uint32_t want = hlit + hdist;
    while (n < want) {
        br.refill();
        const int sym = decode_sym(pre, br);
        if (sym < 0) return kInfBadCode;
        if (sym < 16) { if (lane == 0) lens[20 + n] = static_cast<uint8_t>(sym); prev = static_cast<uint32_t>(sym); n++; continue; }
        uint32_t rep, val = 0;
        br.refill();
        if (sym == 16) { if (n == 0) return kInfBadCode; val = prev; rep = 3 + br.take(2); }
        else if (sym == 17) rep = 3 + br.take(3);
        else rep = 11 + br.take(7);
        if (n + rep > want) return kInfBadCode;
        for (uint32_t i = lane; i < rep; i += 64) lens[20 + n + i] = static_cast<uint8_t>(val);
        n += rep; prev = val;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if (lens[20 + 256] == 0) return kInfBadCode;                               // no end-of-block code
    if (!build_code(lit, lens + 20, static_cast<int>(hlit), true) || !build_code(dist, lens + 20 + hlit, static_cast<int>(hdist), true)) return kInfBadCode;
    return kInfOk;
}

}  // namespace palace
