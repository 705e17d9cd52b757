// One BGZF member written by one workgroup (bgzf_deflate.hip): the text of a member in LDS, tokens from one candidate per byte,
// one dynamic-Huffman block.  The member is built in phases that keep all their state in the workgroup's shared block, so the
// same text compiles for the host as well: host/deflate_selftest_main.cpp runs the phases thread by thread on a CPU and lets zlib
// inflate the result.
//
// Tokens (RFC 1951 3.2.5).  The text is tab-separated lines whose neighbours differ in a digit or two (`samtools depth`): the
// match candidate of a byte is the byte one previous-line-length back, so a line has ONE distance -- the length of the line before
// it -- and a match is found by comparing, not by hashing: nothing depends on the order in which lanes run.  A match has 3 .. 258
// bytes and ends with its line at the latest; the first line of a member, and a line behind one longer than 32 768 bytes, has
// literals only.  Thread t owns the lines that START in bytes [t * chunk, (t + 1) * chunk) and walks each greedily to its end.
// The walk is done three times (histograms; bits per thread; the bits themselves) instead of storing tokens: LDS holds the text
// and a few KiB of tables, 72 KiB in all, so that two workgroups share a CU.
//
// Codes.  Literal/length, distance and code-length codes are Huffman codes of the member's own histograms (in-place
// Moffat-Katajainen on the frequencies sorted by (frequency, symbol)), limited to 15 / 15 / 7 bits by moving codes between the
// length classes until the Kraft sum is exact, and assigned canonically.  A member without a match declares one distance code of
// one bit; a code-length alphabet with one used symbol gets a second one (zlib refuses an incomplete code there).  The header
// lists the code lengths one by one (symbols 16 / 17 / 18 are not used).
//
// Bits.  The member from byte 16 on (BSIZE, the block, CRC-32, ISIZE) is one bit string of kEncSegs segments: segment 0 = BSIZE and
// the block header, segment 1 + t = the tokens of thread t, the last = end-of-block, padding, the trailer.  An exclusive scan of the
// segments' lengths places them.  A dword that lies inside one segment is stored by that segment's thread; a dword that holds a
// border between segments is OR-ed together in LDS, in the slot of the segment that holds the dword's first bit, and stored once.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PALACE_ENC_FN __device__ __forceinline__
#else
#define PALACE_ENC_FN inline
#endif

namespace palace {

constexpr int kEncThreads = 512;
constexpr int kEncSegs = kEncThreads + 2;
constexpr int kEncMaxText = 0xff00;
constexpr int kEncSlot = 65536;

struct EncShared {
    uint32_t text[kEncMaxText / 4 + 2];            // the member's text at byte `mis` (the source's misalignment: whole dwords are copied)
    uint32_t lit_freq[288], dist_freq[32], cl_freq[20];
    uint32_t lit_key[288], dist_key[32], cl_key[20];      // frequencies in ascending order; then code lengths (Moffat-Katajainen)
    uint16_t lit_sorted[288], dist_sorted[32], cl_sorted[20];
    uint16_t lit_code[288], dist_code[32], cl_code[20];   // bit-reversed: ready for an LSB-first bit string
    uint8_t lit_len[288], dist_len[32], cl_len[20];
    uint32_t seg_off[kEncSegs + 1];                // bit offsets of the segments (from byte 16 of the member); [kEncSegs] = all bits
    uint32_t merge[kEncSegs];                      // dwords shared between segments
    int32_t n, mis, chunk, nlit, ndist, nclen, stored;
    uint32_t crc, member_len;
};

#if defined(__HIPCC__)
PALACE_ENC_FN void enc_add(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
PALACE_ENC_FN void enc_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
#else
PALACE_ENC_FN void enc_add(uint32_t *p, uint32_t v) { *p += v; }
PALACE_ENC_FN void enc_or(uint32_t *p, uint32_t v) { *p |= v; }
#endif

PALACE_ENC_FN int enc_log2(uint32_t v) { return 31 - __builtin_clz(v); }
PALACE_ENC_FN uint8_t enc_byte(const EncShared &s, int i) { return reinterpret_cast<const uint8_t *>(s.text)[s.mis + i]; }

// length 3 .. 258 -> code 0 .. 28 (symbol 257 + code), extra bits and their value
PALACE_ENC_FN void enc_len_code(int len, int &code, int &extra, uint32_t &val)
{
    const uint32_t l = static_cast<uint32_t>(len - 3);
    if (len == 258) { code = 28; extra = 0; val = 0; }
    else if (l < 8) { code = static_cast<int>(l); extra = 0; val = 0; }
    else { extra = enc_log2(l) - 2; code = 4 * extra + 4 + static_cast<int>((l >> extra) & 3); val = l & ((1u << extra) - 1); }
}
// distance 1 .. 32768 -> code 0 .. 29
PALACE_ENC_FN void enc_dist_code(int dist, int &code, int &extra, uint32_t &val)
{
    const uint32_t d = static_cast<uint32_t>(dist - 1);
    if (d < 4) { code = static_cast<int>(d); extra = 0; val = 0; }
    else { extra = enc_log2(d) - 1; code = 2 * extra + 2 + static_cast<int>((d >> extra) & 1); val = d & ((1u << extra) - 1); }
}

// The tokens of the lines that start in thread tid's chunk, in text order: f.literal(byte) / f.match(length, distance).
template <class F>
PALACE_ENC_FN void enc_walk(const EncShared &s, int tid, F &f)
{
    const int n = s.n, c0 = tid * s.chunk, c1 = c0 + s.chunk < n ? c0 + s.chunk : n;
    int i = c0;
    if (i > 0)
        while (i < c1 && enc_byte(s, i - 1) != '\n') i++;                  // the first line start in the chunk
    if (i >= c1) return;
    int dist = 0;
    if (i > 0) {                                                           // the line before it: [ps, i)
        int ps = i - 1;
        while (ps > 0 && enc_byte(s, ps - 1) != '\n') ps--;
        dist = i - ps;
    }
    while (i < c1) {                                                       // the line that starts at i
        const bool can = dist > 0 && dist <= 32768;
        int p = i;
        bool open = true;
        while (open && p < n) {
            int r = 0;
            if (can)
                while (r < 258 && p + r < n && enc_byte(s, p + r) == enc_byte(s, p + r - dist)) {
                    r++;
                    if (enc_byte(s, p + r - 1) == '\n') break;
                }
            if (r >= 3) {
                f.match(r, dist);
                p += r;
            } else {
                f.literal(enc_byte(s, p));
                p++;
            }
            open = enc_byte(s, p - 1) != '\n';
        }
        dist = p - i;
        i = p;
    }
}

// A walk is the token source of a member: walk(s, tid, f) calls f.literal / f.match for the tokens of thread tid, in text order, and gives
// the same tokens every time.  The phases below take one; without one they take the lines' (deflate_lz.hpp has the other).
struct EncLineWalk {
    template <class F>
    PALACE_ENC_FN void operator()(const EncShared &s, int tid, F &f) const { enc_walk(s, tid, f); }
};

struct EncCountFreq {
    EncShared &s;
    PALACE_ENC_FN void literal(uint8_t b) { enc_add(&s.lit_freq[b], 1); }
    PALACE_ENC_FN void match(int len, int dist)
    {
        int c, e; uint32_t v;
        enc_len_code(len, c, e, v);
        enc_add(&s.lit_freq[257 + c], 1);
        enc_dist_code(dist, c, e, v);
        enc_add(&s.dist_freq[c], 1);
    }
};

struct EncCountBits {
    const EncShared &s;
    uint32_t bits;
    PALACE_ENC_FN void literal(uint8_t b) { bits += s.lit_len[b]; }
    PALACE_ENC_FN void match(int len, int dist)
    {
        int c, e; uint32_t v;
        enc_len_code(len, c, e, v);
        bits += s.lit_len[257 + c] + e;
        enc_dist_code(dist, c, e, v);
        bits += s.dist_len[c] + e;
    }
};

// the segment that holds bit `bit`: the last one that starts at or before it (empty segments in front of it start there too)
PALACE_ENC_FN int enc_owner(const EncShared &s, uint32_t bit)
{
    int lo = 0, hi = kEncSegs;                                            // first segment with seg_off > bit, in (lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s.seg_off[mid] <= bit) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// bits of one segment, LSB first, into the member's dwords (out = the slot from byte 16 on)
struct EncBitWriter {
    EncShared &s;
    uint32_t *out;
    uint64_t acc;
    int nb;
    uint32_t word;
    bool first;                                                            // the next dword to leave is the segment's first and starts inside it
    PALACE_ENC_FN EncBitWriter(EncShared &s_, uint32_t *out_, uint32_t bit0)
        : s(s_), out(out_), acc(0), nb(static_cast<int>(bit0 & 31)), word(bit0 >> 5), first((bit0 & 31) != 0) {}
    PALACE_ENC_FN void put(uint32_t v, int n)                              // n <= 32, v < 2^n
    {
        acc |= static_cast<uint64_t>(v) << nb;
        nb += n;
        if (nb >= 32) {
            const uint32_t w = static_cast<uint32_t>(acc);
            if (first) { enc_or(&s.merge[enc_owner(s, word * 32)], w); first = false; }
            else out[word] = w;
            acc >>= 32; nb -= 32; word++;
        }
    }
    PALACE_ENC_FN void finish()
    {
        if (acc != 0) enc_or(&s.merge[enc_owner(s, word * 32)], static_cast<uint32_t>(acc));
    }
};

struct EncEmit {
    const EncShared &s;
    EncBitWriter &w;
    PALACE_ENC_FN void literal(uint8_t b) { w.put(s.lit_code[b], s.lit_len[b]); }
    PALACE_ENC_FN void match(int len, int dist)
    {
        int c, e; uint32_t v;
        enc_len_code(len, c, e, v);
        w.put(s.lit_code[257 + c] | (v << s.lit_len[257 + c]), s.lit_len[257 + c] + e);
        enc_dist_code(dist, c, e, v);
        w.put(s.dist_code[c] | (v << s.dist_len[c]), s.dist_len[c] + e);
    }
};

// ---- phases: every thread of the workgroup runs phase k, then all wait, then phase k + 1 -------------------------------------

// (the text is in LDS, n / mis / chunk / crc are set)
PALACE_ENC_FN void enc_phase_clear(EncShared &s, int tid)
{
    for (int i = tid; i < 288; i += kEncThreads) { s.lit_freq[i] = 0; s.lit_len[i] = 0; s.lit_code[i] = 0; }
    if (tid < 32) { s.dist_freq[tid] = 0; s.dist_len[tid] = 0; s.dist_code[tid] = 0; }
    if (tid < 20) { s.cl_freq[tid] = 0; s.cl_len[tid] = 0; s.cl_code[tid] = 0; }
    for (int i = tid; i < kEncSegs; i += kEncThreads) s.merge[i] = 0;
}

template <class W>
PALACE_ENC_FN void enc_phase_freq(EncShared &s, int tid, const W &walk)
{
    EncCountFreq f{s};
    walk(s, tid, f);
    if (tid == 0) enc_add(&s.lit_freq[256], 1);
}
PALACE_ENC_FN void enc_phase_freq(EncShared &s, int tid) { enc_phase_freq(s, tid, EncLineWalk{}); }

// rank of symbol `sym` among the used symbols by (frequency, symbol)
PALACE_ENC_FN void enc_rank(const uint32_t *freq, int n_sym, int sym, uint32_t *key, uint16_t *sorted)
{
    const uint32_t f = freq[sym];
    if (f == 0) return;
    int rank = 0;
    for (int t = 0; t < n_sym; t++) {
        const uint32_t g = freq[t];
        rank += (g != 0 && (g < f || (g == f && t < sym))) ? 1 : 0;
    }
    key[rank] = f;
    sorted[rank] = static_cast<uint16_t>(sym);
}

PALACE_ENC_FN void enc_phase_sort(EncShared &s, int tid)
{
    if (tid < 286) enc_rank(s.lit_freq, 286, tid, s.lit_key, s.lit_sorted);
    else if (tid >= 288 && tid < 288 + 30) enc_rank(s.dist_freq, 30, tid - 288, s.dist_key, s.dist_sorted);
}

// One thread: the code of an alphabet from key[] / sorted[] (ascending), lengths limited to max_bits, codes canonical and reversed.
// Returns the number of used symbols.
PALACE_ENC_FN int enc_build_code(const uint32_t *freq, int n_sym, int max_bits, uint32_t *A, const uint16_t *sorted, uint8_t *len, uint16_t *code)
{
    int n = 0;
    for (int t = 0; t < n_sym; t++) n += freq[t] != 0 ? 1 : 0;
    if (n == 0) return 0;
    uint32_t num[17];
    for (int i = 0; i <= 16; i++) num[i] = 0;
    if (n == 1) {
        num[1] = 1;
    } else {
        A[0] += A[1];
        int root = 0, leaf = 2, next;
        for (next = 1; next < n - 1; next++) {
            if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = static_cast<uint32_t>(next); } else A[next] = A[leaf++];
            if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = static_cast<uint32_t>(next); } else A[next] += A[leaf++];
        }
        A[n - 2] = 0;
        for (next = n - 3; next >= 0; next--) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0;
        root = n - 2; next = n - 1;
        while (avbl > 0) {
            while (root >= 0 && static_cast<int>(A[root]) == dpth) { used++; root--; }
            while (avbl > used) { A[next--] = static_cast<uint32_t>(dpth); avbl--; }
            avbl = 2 * used; dpth++; used = 0;
        }
        for (int i = 0; i < n; i++) num[A[i] < static_cast<uint32_t>(max_bits) ? A[i] : max_bits]++;
        uint32_t total = 0;
        for (int i = max_bits; i > 0; i--) total += num[i] << (max_bits - i);
        while (total != (1u << max_bits)) {                               // too many codes for max_bits: one of the longest leaves, a shorter one takes its sibling
            num[max_bits]--;
            for (int i = max_bits - 1; i > 0; i--)
                if (num[i]) { num[i]--; num[i + 1] += 2; break; }
            total--;
        }
    }
    int j = n;
    for (int i = 1; i <= max_bits; i++)
        for (uint32_t k = num[i]; k > 0; k--) len[sorted[--j]] = static_cast<uint8_t>(i);
    uint32_t next_code[17];
    next_code[1] = 0;
    for (int i = 1; i < max_bits; i++) next_code[i + 1] = (next_code[i] + num[i]) << 1;
    for (int t = 0; t < n_sym; t++) {
        const int l = len[t];
        if (!l) continue;
        uint32_t c = next_code[l]++, r = 0;
        for (int b = 0; b < l; b++) { r = (r << 1) | (c & 1); c >>= 1; }
        code[t] = static_cast<uint16_t>(r);
    }
    return n;
}

PALACE_ENC_FN void enc_phase_codes(EncShared &s, int tid)
{
    if (tid == 0) {
        enc_build_code(s.lit_freq, 286, 15, s.lit_key, s.lit_sorted, s.lit_len, s.lit_code);
        int nlit = 286;
        while (nlit > 257 && s.lit_len[nlit - 1] == 0) nlit--;
        s.nlit = nlit;
    } else if (tid == 64) {
        const int used = enc_build_code(s.dist_freq, 30, 15, s.dist_key, s.dist_sorted, s.dist_len, s.dist_code);
        if (used == 0) s.dist_len[0] = 1;                                 // no match: one distance code, never sent
        int ndist = 30;
        while (ndist > 1 && s.dist_len[ndist - 1] == 0) ndist--;
        s.ndist = ndist;
    }
}

PALACE_ENC_FN void enc_phase_cl_freq(EncShared &s, int tid)
{
    for (int i = tid; i < s.nlit + s.ndist; i += kEncThreads) enc_add(&s.cl_freq[i < s.nlit ? s.lit_len[i] : s.dist_len[i - s.nlit]], 1);
}

#if defined(__HIPCC__)
static __device__ const uint8_t kEncClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
#else
static const uint8_t kEncClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
#endif
PALACE_ENC_FN const uint8_t *enc_cl_order() { return kEncClOrder; }

PALACE_ENC_FN void enc_phase_cl_code(EncShared &s, int tid)
{
    if (tid != 0) return;
    int used = 0;
    for (int t = 0; t < 19; t++) used += s.cl_freq[t] != 0 ? 1 : 0;
    int dummy = -1;
    if (used == 1) { dummy = s.cl_freq[0] ? 1 : 0; s.cl_freq[dummy] = 1; }   // zlib refuses an incomplete code here: a second symbol that is never sent
    for (int t = 0; t < 19; t++) enc_rank(s.cl_freq, 19, t, s.cl_key, s.cl_sorted);
    enc_build_code(s.cl_freq, 19, 7, s.cl_key, s.cl_sorted, s.cl_len, s.cl_code);
    if (dummy >= 0) s.cl_freq[dummy] = 0;
    const uint8_t *order = enc_cl_order();
    int nclen = 19;
    while (nclen > 4 && s.cl_len[order[nclen - 1]] == 0) nclen--;
    s.nclen = nclen;
    uint32_t bits = 16 + 3 + 5 + 5 + 4 + 3 * static_cast<uint32_t>(nclen);
    for (int t = 0; t < 19; t++) bits += s.cl_freq[t] * s.cl_len[t];
    s.seg_off[0] = bits;                                                  // lengths until the scan
}

template <class W>
PALACE_ENC_FN uint32_t enc_token_bits(const EncShared &s, int tid, const W &walk)
{
    EncCountBits f{s, 0};
    walk(s, tid, f);
    return f.bits;
}

template <class W>
PALACE_ENC_FN void enc_phase_bits(EncShared &s, int tid, const W &walk) { s.seg_off[1 + tid] = enc_token_bits(s, tid, walk); }
PALACE_ENC_FN void enc_phase_bits(EncShared &s, int tid) { enc_phase_bits(s, tid, EncLineWalk{}); }

// one thread (the device runs a workgroup scan in its place): lengths -> offsets; stored or coded; the member's length
PALACE_ENC_FN void enc_finish_scan(EncShared &s, uint32_t token_bits_end)
{
    const uint32_t eob_end = token_bits_end + s.lit_len[256];
    const uint32_t padded = (eob_end + 7) & ~7u;
    s.seg_off[kEncSegs - 1] = token_bits_end;
    s.seg_off[kEncSegs] = padded + 64;
    const uint32_t coded = padded / 8 - 2;                                // bytes of the DEFLATE stream
    s.stored = coded >= 5u + static_cast<uint32_t>(s.n) ? 1 : 0;
    s.member_len = s.stored ? 18u + 5u + static_cast<uint32_t>(s.n) + 8u : 16u + s.seg_off[kEncSegs] / 8;
}

PALACE_ENC_FN void enc_scan_serial(EncShared &s)
{
    uint32_t at = 0;
    for (int k = 0; k < kEncSegs - 1; k++) { const uint32_t b = s.seg_off[k]; s.seg_off[k] = at; at += b; }
    enc_finish_scan(s, at);
}

PALACE_ENC_FN uint8_t enc_stored_byte(const EncShared &s, uint32_t k)     // byte k of a member written as a stored block, k >= 16
{
    const uint32_t n = static_cast<uint32_t>(s.n), bsize = s.member_len - 1;
    if (k < 18) return static_cast<uint8_t>(bsize >> (8 * (k - 16)));
    if (k == 18) return 1;                                                // BFINAL = 1, BTYPE = 00, padding
    if (k < 21) return static_cast<uint8_t>(n >> (8 * (k - 19)));
    if (k < 23) return static_cast<uint8_t>(~n >> (8 * (k - 21)));
    if (k < 23 + n) return enc_byte(s, static_cast<int>(k - 23));
    if (k < 27 + n) return static_cast<uint8_t>(s.crc >> (8 * (k - 23 - n)));
    if (k < 31 + n) return static_cast<uint8_t>(n >> (8 * (k - 27 - n)));
    return 0;
}

// slot: the member's 65 536 bytes as dwords
template <class W>
PALACE_ENC_FN void enc_phase_write(EncShared &s, int tid, uint32_t *slot, const W &walk)
{
    if (tid < 4) {
        const uint32_t head[4] = {0x04088b1fu, 0u, 0x0006ff00u, 0x00024342u};  // 1f 8b 08 04 | mtime | xfl 00, os ff, xlen 6 | 'B' 'C' 2 0
        slot[tid] = head[tid];
    }
    if (s.stored) {
        for (uint32_t d = 4 + static_cast<uint32_t>(tid); d * 4 < s.member_len; d += kEncThreads) {
            uint32_t w = 0;
            for (uint32_t b = 0; b < 4; b++) w |= static_cast<uint32_t>(enc_stored_byte(s, d * 4 + b)) << (8 * b);
            slot[d] = w;
        }
        return;
    }
    uint32_t *out = slot + 4;
    {
        EncBitWriter w(s, out, s.seg_off[1 + tid]);
        EncEmit f{s, w};
        walk(s, tid, f);
        w.finish();
    }
    if (tid == 0) {                                                       // BSIZE and the block header
        EncBitWriter w(s, out, 0);
        w.put(s.member_len - 1, 16);
        w.put(5, 3);                                                      // BFINAL = 1, BTYPE = 10
        w.put(static_cast<uint32_t>(s.nlit - 257), 5);
        w.put(static_cast<uint32_t>(s.ndist - 1), 5);
        w.put(static_cast<uint32_t>(s.nclen - 4), 4);
        const uint8_t *order = enc_cl_order();
        for (int k = 0; k < s.nclen; k++) w.put(s.cl_len[order[k]], 3);
        for (int i = 0; i < s.nlit + s.ndist; i++) {
            const int l = i < s.nlit ? s.lit_len[i] : s.dist_len[i - s.nlit];
            w.put(s.cl_code[l], s.cl_len[l]);
        }
        w.finish();
    }
    if (tid == kEncThreads - 1) {                                         // end of block, padding, CRC-32, ISIZE
        const uint32_t b0 = s.seg_off[kEncSegs - 1];
        EncBitWriter w(s, out, b0);
        w.put(s.lit_code[256], s.lit_len[256]);
        const uint32_t at = b0 + s.lit_len[256];
        w.put(0, static_cast<int>(((at + 7) & ~7u) - at));
        w.put(s.crc, 32);
        w.put(static_cast<uint32_t>(s.n), 32);
        w.finish();
    }
}
PALACE_ENC_FN void enc_phase_write(EncShared &s, int tid, uint32_t *slot) { enc_phase_write(s, tid, slot, EncLineWalk{}); }

// the dwords that were put together in LDS: segment k stores the one it ends in, if it holds that dword's first bit
PALACE_ENC_FN void enc_phase_merge(EncShared &s, int tid, uint32_t *slot)
{
    if (s.stored) return;
    for (int k = tid; k < kEncSegs; k += kEncThreads) {
        const uint32_t b0 = s.seg_off[k], b1 = s.seg_off[k + 1];
        if (b1 > b0 && (b1 & 31) != 0 && b0 <= (b1 & ~31u)) slot[4 + (b1 >> 5)] = s.merge[k];
    }
}

// an empty piece: the 28-byte member that also ends a BGZF file
PALACE_ENC_FN void enc_write_empty(int tid, uint32_t *slot)
{
    const uint32_t eof[7] = {0x04088b1fu, 0u, 0x0006ff00u, 0x00024342u, 0x0003001bu, 0u, 0u};
    if (tid < 7) slot[tid] = eof[tid];
}

}  // namespace palace
