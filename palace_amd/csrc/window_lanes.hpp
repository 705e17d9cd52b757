// What the writers of an output text (paths_writer.hpp, fastg_split.hip, readqc.hip) share.  A plan gave every item of the output -- a
// path, a record, a read pair -- its byte offset; a writer kernel makes any window [lo, hi) of the text, a lane 16 aligned bytes of it:
//   the lane of a window: which bytes a lane owes, the item of its first byte (searched between the items of the tile's first and last
//       byte, which are searched once per tile), the bytes gathered in two registers and stored once;
//   the bases of one indexed FASTA record, from any place, on either strand: 16 neighbours of one source line are one load and one
//       store, anything else a walk byte by byte that steps over the line ends;
//   the three complements of the reference's scripts.
// Device only.
#pragma once
#include "scan64.hpp"

namespace palace {
namespace {

constexpr int kTileThreads = 256, kTileBytes = kTileThreads * kLaneBytes;

// ---- the lane of a window -----------------------------------------------------------------------------------------------------------

struct LaneOut {
    int64_t j0, o0;                          // the lane's first byte: in the window's buffer, in the whole text
    int cnt, k;                              // the bytes it owes (16, fewer at the window's end) and those it has
    uint64_t acc_lo, acc_hi;
    __device__ __forceinline__ void put(uint32_t b)
    {
        if (k < 8) acc_lo |= static_cast<uint64_t>(b) << (8 * k); else acc_hi |= static_cast<uint64_t>(b) << (8 * (k - 8));
        k++;
    }
    __device__ __forceinline__ bool full() const { return k >= cnt; }
    __device__ __forceinline__ void store(uint8_t *out) const
    {
        if (cnt == kLaneBytes)
            *reinterpret_cast<uint4 *>(out + j0) = make_uint4(static_cast<uint32_t>(acc_lo), static_cast<uint32_t>(acc_lo >> 32), static_cast<uint32_t>(acc_hi),
                                                              static_cast<uint32_t>(acc_hi >> 32));
        else
            for (int i = 0; i < cnt; i++) out[j0 + i] = static_cast<uint8_t>((i < 8 ? acc_lo >> (8 * i) : acc_hi >> (8 * (i - 8))) & 0xffu);
    }
};

// The lane's share of the window [lo, hi) of a text whose item i begins at off[i] (off[0 .. n_items], off[0] = 0 <= lo < hi), and the
// item of its first byte: the last of equal entries, so an item with text.  -1 for a lane behind the window's end, which has nothing
// to do -- but every lane of the workgroup comes here, there is a barrier inside.  s_item: two words of the workgroup's LDS.
__device__ __forceinline__ int64_t window_lane(const int64_t *off, int64_t n_items, int64_t lo, int64_t hi, long long *s_item, LaneOut *lane)
{
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTileBytes;
    if (threadIdx.x < 2) {                                                   // the items of the tile's first and last byte
        const int64_t end = lo + tile0 + kTileBytes < hi ? lo + tile0 + kTileBytes : hi;
        s_item[threadIdx.x] = last_le(off, 0, n_items - 1, threadIdx.x == 0 ? lo + tile0 : end - 1);
    }
    __syncthreads();
    const int64_t j0 = tile0 + threadIdx.x * kLaneBytes, o0 = lo + j0;
    if (o0 >= hi) return -1;
    *lane = LaneOut{j0, o0, hi - o0 < kLaneBytes ? static_cast<int>(hi - o0) : kLaneBytes, 0, 0, 0};
    return last_le(off, s_item[0], s_item[1], o0);
}

// the bytes of `>name LF` from place x on, as many as the lane still takes; x moves with them
__device__ __forceinline__ void put_header(LaneOut &l, const uint8_t *name, int64_t h, int64_t &x)
{
    for (; !l.full() && x < h + 2; x++) l.put(x == 0 ? '>' : x == h + 1 ? '\n' : name[x - 1]);
}

// ---- the bases of one record ----------------------------------------------------------------------------------------------------------

template <class Comp>
__device__ __forceinline__ uint32_t complement4(Comp comp, uint32_t w)
{
    return comp(w & 0xffu) | (comp((w >> 8) & 0xffu) << 8) | (comp((w >> 16) & 0xffu) << 16) | (comp(w >> 24) << 24);
}

// m bases (0 < m <= the lane's room) of the bases [start, start + span) of record r of the indexed text (r.line_bases > 0: a select
// in front of the division is a measurable part of the paths writer's time), from place pos_in_seq of that range on; rev: of its
// other strand, read from the range's end through comp.  True: they were the lane's whole 16 bytes and 16 neighbours of one source
// line, and are stored already -- one load, one store; the lane is done.  False: they are put.
template <class Comp>
__device__ __forceinline__ bool gather_bases(LaneOut &l, const uint8_t *text, const palace_fasta_rec &r, int64_t start, int64_t span, int64_t pos_in_seq, int m,
                                             bool rev, uint8_t *out, Comp comp)
{
    const int64_t pos = start + (rev ? span - 1 - pos_in_seq : pos_in_seq);
    const int64_t line_bases = r.line_bases;                                 // (> 0: an indexed record with bases has a first line)
    const int64_t row = pos / line_bases;
    int64_t col = pos - row * line_bases, src = r.seq_off + row * r.line_width + col;
    if (m == kLaneBytes && (rev ? col >= kLaneBytes - 1 : col + kLaneBytes <= line_bases)) {
        uint4 v;
        __builtin_memcpy(&v, text + (rev ? src - (kLaneBytes - 1) : src), sizeof v);
        if (rev)
            v = make_uint4(__builtin_bswap32(complement4(comp, v.w)), __builtin_bswap32(complement4(comp, v.z)), __builtin_bswap32(complement4(comp, v.y)),
                           __builtin_bswap32(complement4(comp, v.x)));
        *reinterpret_cast<uint4 *>(out + l.j0) = v;
        return true;
    }
    const int64_t gap = r.line_width - line_bases;
    for (int i = 0; i < m; i++) {
        const uint32_t b = text[src];
        l.put(rev ? comp(b) : b);
        if (rev) { if (col == 0) { col = line_bases - 1; src -= gap + 1; } else { col--; src--; } }
        else if (++col == line_bases) { col = 0; src += gap + 1; } else src++;
    }
    return false;
}

// the same of the whole record
template <class Comp>
__device__ __forceinline__ bool gather_bases(LaneOut &l, const uint8_t *text, const palace_fasta_rec &r, int64_t pos_in_seq, int m, bool rev, uint8_t *out,
                                             Comp comp)
{
    return gather_bases(l, text, r, 0, r.length, pos_in_seq, m, rev, out, comp);
}

// ---- the complements: three, as the reference's scripts differ ------------------------------------------------------------------------

// make_fa_from_path: A<->T, C<->G in either case; every other byte as it is
struct ComplementAcgt {
    __device__ __forceinline__ uint32_t operator()(uint32_t b) const
    {
        const uint32_t u = b & 0xdfu;
        return b ^ ((u == 'A' || u == 'T') ? 0x15u : (u == 'C' || u == 'G') ? 0x04u : 0u);
    }
};

// make_final_fa: Biopython's ambiguous-DNA complement as the XOR of a letter's low five bits: A<->T, C<->G, R<->Y, K<->M, B<->V, D<->H;
// S, W, N and every other byte stay.  The same in either case.
__constant__ const uint8_t kCompXor[32] = {
    0,
    'A' ^ 'T', 'B' ^ 'V', 'C' ^ 'G', 'D' ^ 'H', 0, 0, 'G' ^ 'C', 'H' ^ 'D', 0, 0, 'K' ^ 'M', 0, 'M' ^ 'K',   // A .. M
    0, 0, 0, 0, 'R' ^ 'Y', 0, 'T' ^ 'A', 0, 'V' ^ 'B', 0, 0, 'Y' ^ 'R', 0,                                   // N .. Z
    0, 0, 0, 0, 0};
struct ComplementAmbiguous {
    __device__ __forceinline__ uint32_t operator()(uint32_t b) const { return (b & 0xc0u) == 0x40u ? b ^ kCompXor[b & 0x1fu] : b; }
};

// split_fastg: the other strand's base in upper case, A<->T, C<->G in either case (a primed record holds nothing else)
struct ComplementUpper {
    __device__ __forceinline__ uint32_t operator()(uint32_t b) const
    {
        const uint32_t u = b & 0xdfu;
        return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u ^ ((u == 'A' || u == 'T') ? 0x15u : 0x04u) : b;
    }
};

}  // namespace
}  // namespace palace
