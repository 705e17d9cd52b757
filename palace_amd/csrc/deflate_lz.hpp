// A second token source for the member writer of deflate_enc.hpp (bgzf_deflate.hip: palace_bgzf_deflate_lz): matches found through a
// hash of the next four bytes instead of the previous line, for text without lines -- the records of a BAM.  Everything behind the
// tokens (length and distance codes, the Huffman codes and their limit, the header, the segment scan, the bit writer, the merge of
// border dwords, the stored fallback, the empty member) is deflate_enc.hpp's, with this walk in the place of enc_walk.  Like that
// header this one compiles for the host: host/deflate_lz_selftest_main.cpp runs the phases thread by thread on a CPU.
//
// The rule.  It is a function of the member's n bytes alone; R = kEncThreads = 512.
//   Hash.       h(p) = (the little-endian 32-bit word of bytes p .. p + 3) * 2654435761 mod 2^32, its top 14 bits; defined for
//               p <= n - 4.
//   Candidate.  The member is taken in rounds of R consecutive positions; the round of p begins at R * floor(p / R).  cand(p) is the
//               greatest q with h(q) == h(p), q < R * floor(p / R) and p - q <= 32768, or none.  (The greatest q with the first two
//               properties either has the third or no q has.)  A position has NO candidate inside its own round -- a repeat
//               whose source lies less than p mod R + 1 bytes back is not found -- and the last three positions of a member have none.
//               What is kept is the distance dist(p) = p - cand(p), 1 .. 32768, or 0 for none.
//   Tokens.     Thread t owns the bytes [t * chunk, (t + 1) * chunk), chunk = ceil(n / R), and parses them greedily from its first
//               byte: at p the match length is the number of equal bytes text[p + k] == text[p + k - dist(p)], capped at 258, at the
//               member's end and at the chunk's end; 3 or more is a match (length, dist(p)) and parsing resumes behind it, fewer is
//               the literal text[p].  No token straddles a chunk border, so chunks are independent.  A copy may overlap what it
//               writes (distance < length).  Bytes with equal hash and different text compare unequal and become literals.
//               (chunk <= 128 for n <= 0xff00, so the cap of 258 never binds: a longer repeat is several tokens, one per chunk.)
//
// On the device the candidates come from a head table in LDS (per bucket the greatest position so far, + 1): per round every lane
// reads the bucket of its position, all wait, every lane raises it with an atomic max, all wait.  The result of a max does not
// depend on the order of the lanes.  Text (65 KiB) and a distance per position (128 KiB) do not fit the 160 KiB of a CU's LDS
// together, so the distances go to device memory, 2 bytes per text byte, kLzDistBytes per resident workgroup, and the three walks
// (histograms; bits per thread; the bits) read them back.  LDS: EncShared + 64 KiB of head table = 137 KiB, one workgroup per CU.
#pragma once
#include <cstddef>

#include "deflate_enc.hpp"

namespace palace {

constexpr int kLzHashBits = 14;
constexpr int kLzBuckets = 1 << kLzHashBits;
constexpr int kLzWindow = 32768;
constexpr size_t kLzDistBytes = 2 * static_cast<size_t>(kEncSlot);       // uint16 dist[p], p < n <= 0xff00

struct LzShared {
    EncShared e;
    uint32_t head[kLzBuckets];                     // greatest position with this hash in the rounds before the current one, + 1; 0 = none
};

#if defined(__HIPCC__)
PALACE_ENC_FN void lz_max(uint32_t *p, uint32_t v) { atomicMax(p, v); }
#else
PALACE_ENC_FN void lz_max(uint32_t *p, uint32_t v) { if (*p < v) *p = v; }
#endif

PALACE_ENC_FN uint32_t lz_hash(const EncShared &s, int p)               // p <= n - 4
{
    const uint32_t w = static_cast<uint32_t>(enc_byte(s, p)) | static_cast<uint32_t>(enc_byte(s, p + 1)) << 8 |
                       static_cast<uint32_t>(enc_byte(s, p + 2)) << 16 | static_cast<uint32_t>(enc_byte(s, p + 3)) << 24;
    return (w * 2654435761u) >> (32 - kLzHashBits);
}

PALACE_ENC_FN void lz_phase_clear(LzShared &s, int tid)
{
    for (int i = tid; i < kLzBuckets; i += kEncThreads) s.head[i] = 0;
}

PALACE_ENC_FN int lz_rounds(const EncShared &s) { return (s.n + kEncThreads - 1) / kEncThreads; }

// round r, first half: dist(p) of p = r * R + tid from the table as the rounds before r left it
PALACE_ENC_FN void lz_phase_look(const LzShared &s, int tid, int r, uint16_t *dist)
{
    const int p = r * kEncThreads + tid;
    if (p >= s.e.n) return;
    uint32_t d = 0;
    if (p + 4 <= s.e.n) {
        const uint32_t q1 = s.head[lz_hash(s.e, p)];
        if (q1 != 0 && static_cast<uint32_t>(p) + 1 - q1 <= static_cast<uint32_t>(kLzWindow)) d = static_cast<uint32_t>(p) + 1 - q1;
    }
    dist[p] = static_cast<uint16_t>(d);
}

// round r, second half (after every lane has looked): p enters the table
PALACE_ENC_FN void lz_phase_enter(LzShared &s, int tid, int r)
{
    const int p = r * kEncThreads + tid;
    if (p + 4 <= s.e.n) lz_max(&s.head[lz_hash(s.e, p)], static_cast<uint32_t>(p) + 1);
}

// The tokens of thread tid's chunk, in text order.  dist: the member's distances, n entries.
struct LzWalk {
    const uint16_t *dist;
    template <class F>
    PALACE_ENC_FN void operator()(const EncShared &s, int tid, F &f) const
    {
        const int c0 = tid * s.chunk, c1 = c0 + s.chunk < s.n ? c0 + s.chunk : s.n;
        int p = c0;
        while (p < c1) {
            const int d = dist[p];
            int r = 0;
            if (d) {
                const int cap = c1 - p < 258 ? c1 - p : 258;
                while (r < cap && enc_byte(s, p + r) == enc_byte(s, p + r - d)) r++;
            }
            if (r >= 3) {
                f.match(r, d);
                p += r;
            } else {
                f.literal(enc_byte(s, p));
                p++;
            }
        }
    }
};

}  // namespace palace
