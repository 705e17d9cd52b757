// The host's share of a gzip member (RFC 1952) for the device inflater (csrc/gzip.hip): where the DEFLATE data behind a member's
// header begin, and the running CRC-32 / ISIZE of a member put together from the CRCs of its chunks.  No device code: builds on a CPU.
#pragma once
#include <zlib.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace palace_host {

// Offset of the first byte of DEFLATE data of the member whose header starts at `pos`, or -1 for a header zlib would refuse
// (no magic, a method other than 8, reserved flag bits, a header CRC that does not match) or that the file cuts short.
inline int64_t gzip_header_end(const uint8_t *file, size_t size, size_t pos)
{
    if (size < pos || size - pos < 10) return -1;
    const uint8_t *h = file + pos;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || (h[3] & 0xe0)) return -1;
    const int flg = h[3];
    size_t p = pos + 10;
    if (flg & 4) {                                                            // FEXTRA
        if (size - p < 2) return -1;
        const size_t xlen = file[p] | (static_cast<size_t>(file[p + 1]) << 8);
        p += 2;
        if (size - p < xlen) return -1;
        p += xlen;
    }
    for (int bit : {8, 16}) {                                                 // FNAME, FCOMMENT: zero-terminated
        if (!(flg & bit)) continue;
        const void *z = std::memchr(file + p, 0, size - p);
        if (!z) return -1;
        p = static_cast<size_t>(static_cast<const uint8_t *>(z) - file) + 1;
    }
    if (flg & 2) {                                                            // FHCRC: the low 16 bits of the header's CRC-32
        if (size - p < 2) return -1;
        const uint32_t want = file[p] | (static_cast<uint32_t>(file[p + 1]) << 8);
        if ((crc32(0, file + pos, static_cast<uInt>(p - pos)) & 0xffffu) != want) return -1;
        p += 2;
    }
    return static_cast<int64_t>(p);
}

// CRC-32 and length of a member whose text arrives as consecutive ranges, each with a CRC of its own
struct MemberCheck {
    uint32_t crc = 0;
    uint64_t len = 0;
    void add(uint32_t range_crc, int64_t range_len)
    {
        crc = static_cast<uint32_t>(crc32_combine(crc, range_crc, static_cast<z_off_t>(range_len)));
        len += static_cast<uint64_t>(range_len);
    }
    // against the member's trailer (CRC32, ISIZE; little endian): 0 = both match, 1 = the CRC differs, 2 = the size does
    int verdict(const uint8_t *trailer) const
    {
        uint32_t want_crc, want_len;
        std::memcpy(&want_crc, trailer, 4);
        std::memcpy(&want_len, trailer + 4, 4);
        if (crc != want_crc) return 1;
        return static_cast<uint32_t>(len) == want_len ? 0 : 2;
    }
    void reset() { crc = 0; len = 0; }
};

// ---- the chain of chunks inside one span of compressed bytes (csrc/gzip.hip runs it between its kernels) ------------------------------
struct GzChunk {
    int64_t start, stop;                         // bits from the span's first byte: decode from `start` to the first block boundary >= stop
    int64_t out_off, out_len;                    // symbols: where they go, and how many the size pass counted
    int32_t first, pad;                          // the chunk opens a member: nothing lies before it
};
struct GzResult {
    int64_t out_len, end_bit;
    int32_t fin, status;                         // fin: a final block ended the chunk; status: 0, or the decoder's refusal
    int64_t reach;                               // how far the chunk's matches reach before its own first byte (the largest distance - position; 0: not at all)
};
constexpr int32_t kGzOk = 0, kGzNeedsInput = 6;  // (= kInfOk, kInfInput of the device decoder)
struct GzAccepted {                              // a chunk on the chain
    int64_t start, end, out_len;
    int32_t first;
    int64_t trailer;                             // >= 0: the member ends with this chunk; its trailer's file offset
};
struct GzSpan {
    const uint8_t *file;
    int64_t size;                                // of the file
    int64_t a, end_bits;                         // the span: its first byte in the file, its length in bits
    bool at_eof;                                 // it reaches the end of the file
    int64_t cap;                                 // most text of one chunk
    int max_rounds;                              // starts that may be queued behind the first size pass
};
struct GzChainState {
    int64_t pos;                                 // the next certain start (bits from the span's first byte)
    int32_t first;                               // ... opens a member
    bool file_done;
    int64_t member_text = 0;                     // text of the member `pos` lies in, before `pos` (carried from span to span, as `first` is)
    int64_t false_hits = 0, rounds = 0, members = 0;
};
enum { kGzWhyHeader = 1, kGzWhyDecode = 2, kGzWhyChainOpen = 3, kGzWhyNoProgress = 4, kGzWhyTooBig = 5, kGzWhyTruncated = 6, kGzWhyTrailing = 9, kGzWhyMarker = 11 };

// Walks the chain from st.pos over the sized candidates ch / res (ascending starts): a chunk is accepted when it starts where its
// predecessor ended; candidates the chain ran across are false hits; a position without a candidate is sized alone through
// size_one(chunk, &result) (non-zero = a device error, handed back in *device_rc).  Behind a final block the trailer and the next
// member's header are parsed here.  Ends at the end of the file, or at the chunk whose block ends behind the span (st.pos: where the
// next span starts).  A chunk whose matches reach further back than its member has text before it (GzResult::reach against the running
// count st.member_text) refers to bytes before the member's start: zlib's "invalid distance too far back", declined as kGzWhyMarker --
// the window the chunk would be resolved through holds zeros or the previous member's text there, and only the CRC would stand against it.
// Returns 0, or why the file is declined (PALACE_GZ_*); -1 with *device_rc set.
template <class SizeOne>
int gz_chain_walk(const GzSpan &sp, const std::vector<GzChunk> &ch, const std::vector<GzResult> &res, GzChainState &st,
                  std::vector<GzAccepted> &acc, SizeOne &&size_one, int *device_rc)
{
    acc.clear();
    size_t i = 0;
    int rounds = 0;
    while (!st.file_done) {
        while (i < ch.size() && ch[i].start < st.pos) { i++; st.false_hits++; }
        GzChunk c;
        GzResult r;
        if (i < ch.size() && ch[i].start == st.pos) { c = ch[i]; r = res[i]; i++; }
        else {
            if (st.pos >= sp.end_bits) break;                                  // (the next member's header ends behind the span)
            if (rounds == sp.max_rounds) return kGzWhyChainOpen;
            rounds++; st.rounds++;
            c = GzChunk{st.pos, i < ch.size() ? ch[i].start : sp.end_bits, 0, 0, 0, 0};
            if (int rc = size_one(c, &r)) { *device_rc = rc; return -1; }
        }
        if (r.status == kGzNeedsInput) {
            if (sp.at_eof) return kGzWhyTruncated;
            break;                                                             // its block ends behind the span: the next one starts here
        }
        if (r.status != kGzOk || r.end_bit <= c.start) return kGzWhyDecode;
        if (r.out_len > sp.cap) return kGzWhyTooBig;
        if (r.reach > st.member_text) return kGzWhyMarker;
        GzAccepted ac{c.start, r.end_bit, r.out_len, st.first, -1};
        if (r.fin) {
            const int64_t tb = sp.a + ((r.end_bit + 7) >> 3);
            if (tb + 8 > sp.size) return kGzWhyTruncated;
            ac.trailer = tb;
            st.members++;
            if (tb + 8 == sp.size) st.file_done = true;
            else {
                const int64_t hdr = gzip_header_end(sp.file, static_cast<size_t>(sp.size), static_cast<size_t>(tb + 8));
                if (hdr < 0) return sp.file[tb + 8] == 0x1f && sp.size - tb - 8 >= 2 && sp.file[tb + 9] == 0x8b ? kGzWhyHeader : kGzWhyTrailing;
                st.pos = hdr * 8 - sp.a * 8;
                st.first = 1;
            }
            st.member_text = 0;
        } else {
            st.pos = r.end_bit;
            st.first = 0;
            st.member_text += r.out_len;
        }
        acc.push_back(ac);
    }
    return acc.empty() ? kGzWhyNoProgress : 0;
}

}  // namespace palace_host
