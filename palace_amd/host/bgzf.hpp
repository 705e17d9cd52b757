// BGZF (SAM spec 4.1): gzip members with a BC extra subfield carrying the member size, each holding at most 64 KiB of data.  The one
// place the host knows the format: the checked member index, the member decode (the loader's own decoder, zlib behind it) and the
// member writer.
#pragma once
#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "inflate_fast.hpp"

namespace palace_host {

// One member: raw DEFLATE data [in_off, in_off + in_len) of the file, ISIZE = out_len bytes at out_off of the inflated stream.
struct BgzfMember { uint64_t in_off, in_len, out_off, out_len; };

// The members of a mapped file.  Every field that comes from the file is checked against the file before it is used: a member is
// 12 + XLEN header bytes, the deflate stream and an 8-byte trailer, BSIZE + 1 bytes in all.  Fewer than 18 bytes behind the last
// member are ignored (like a missing EOF member).  Throws std::runtime_error.  walk_end (optional): the offset the walk stopped at
// -- of the member it threw on, or behind the last member -- and whether it threw because that member is no BGZF member at all.
struct BgzfWalkEnd { size_t offset = 0; bool not_bgzf = false; };
inline std::vector<BgzfMember> bgzf_members(const uint8_t *file, size_t file_size, size_t *total_out, BgzfWalkEnd *walk_end = nullptr)
{
    auto le16 = [](const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; };
    auto le32 = [](const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; };
    std::vector<BgzfMember> members;
    size_t p = 0, total = 0;
    while (p + 18 <= file_size) {
        const uint8_t *h = file + p;
        if (walk_end) { walk_end->offset = p; walk_end->not_bgzf = true; }
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) throw std::runtime_error("Failed to read BAM header");
        const size_t xlen = le16(h + 10), left = file_size - p;
        if (12 + xlen + 8 > left) throw std::runtime_error("truncated BGZF block");
        size_t q = 12, bsize = 0;
        while (q + 4 <= 12 + xlen) {
            const size_t slen = le16(h + q + 2);
            if (q + 4 + slen > 12 + xlen) throw std::runtime_error("malformed BGZF extra field");
            if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2) bsize = static_cast<size_t>(le16(h + q + 4)) + 1;
            q += 4 + slen;
        }
        if (walk_end) walk_end->not_bgzf = bsize == 0;                       // no BC subfield
        if (bsize < 12 + xlen + 8 || bsize > left) throw std::runtime_error("truncated BGZF block");
        const size_t isize = le32(h + bsize - 4);
        if (isize > 65536) throw std::runtime_error("malformed BGZF block (ISIZE > 64 KiB)");
        members.push_back({p + 12 + xlen, bsize - xlen - 20, total, isize});
        total += isize;
        p += bsize;
    }
    if (walk_end) { walk_end->offset = p; walk_end->not_bgzf = false; }
    *total_out = total;
    return members;
}

// Member m of the file into out[0, m.out_len): the decoder written for the loader first (inflate_fast.hpp; fast = false skips it),
// zlib for whatever it refuses.  zs: a raw inflate stream of the caller's (inflateInit2 with -15), reset and reused here -- or
// nullptr for one of this call's own.  False: zlib refused the member too.
inline bool inflate_member(const uint8_t *file, size_t size, const BgzfMember &m, uint8_t *out, z_stream *zs = nullptr, bool fast = true)
{
    if (m.out_len == 0) return true;
    if (fast && inflate_fast(file + m.in_off, m.in_len, size - (m.in_off + m.in_len), out, m.out_len)) return true;
    z_stream own{};
    if (zs ? inflateReset(zs) != Z_OK : inflateInit2(&own, -15) != Z_OK) return false;
    z_stream &z = zs ? *zs : own;
    z.next_in = const_cast<Bytef *>(file + m.in_off);
    z.avail_in = static_cast<uInt>(m.in_len);
    z.next_out = out;
    z.avail_out = static_cast<uInt>(m.out_len);
    const bool ok = inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_out == 0;
    if (!zs) inflateEnd(&own);
    return ok;
}

constexpr size_t kBgzfText = 0xff00;                   // bytes of data per member as bgzip cuts them (bgzf.h BGZF_BLOCK_SIZE)

// One member for `n` (<= kBgzfText) bytes of data, appended to `out` (raw DEFLATE at `level`, window 2^15, memLevel 8, default
// strategy); throws when zlib fails or the member would not fit 64 KiB.
inline void bgzf_member(const uint8_t *text, size_t n, int level, std::vector<uint8_t> &out)
{
    auto put_le32 = [&out](uint32_t v) { for (int k = 0; k < 4; k++) out.push_back(static_cast<uint8_t>(v >> (8 * k))); };
    static const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    const size_t at = out.size();
    out.insert(out.end(), head, head + 16);
    out.push_back(0); out.push_back(0);                                      // BSIZE, patched below
    z_stream zs{};
    if (deflateInit2(&zs, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) throw std::runtime_error("deflateInit2 failed");
    const size_t bound = deflateBound(&zs, static_cast<uLong>(n));
    out.resize(at + 18 + bound);
    zs.next_in = const_cast<Bytef *>(text); zs.avail_in = static_cast<uInt>(n);
    zs.next_out = out.data() + at + 18; zs.avail_out = static_cast<uInt>(bound);
    const int rc = deflate(&zs, Z_FINISH);
    const size_t clen = bound - zs.avail_out;
    deflateEnd(&zs);
    if (rc != Z_STREAM_END) throw std::runtime_error("deflate failed");
    out.resize(at + 18 + clen);
    put_le32(static_cast<uint32_t>(crc32(crc32(0L, Z_NULL, 0), text, static_cast<uInt>(n))));
    put_le32(static_cast<uint32_t>(n));
    const size_t total = out.size() - at;
    if (total > 0x10000) throw std::runtime_error("BGZF member larger than 64 KiB");
    out[at + 16] = static_cast<uint8_t>(total - 1); out[at + 17] = static_cast<uint8_t>((total - 1) >> 8);
}

// The 28-byte empty member that ends a BGZF file.
inline const uint8_t *bgzf_eof_member()
{
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return eof;
}

}  // namespace palace_host
