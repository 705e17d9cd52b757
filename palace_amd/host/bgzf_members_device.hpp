// Text that lies in device memory written as the members of a BGZF file (`bamsort`, `samview`, `bamdepth --depth-gz-gpu`): members of
// kBgzfText = 0xff00 bytes of text, the last one shorter, a batch at a time -- palace_crc32_members for the trailers,
// palace_bgzf_deflate and palace_bgzf_compact for the members, one copy back per batch, fwrite.  A batch's text is either a piece of a
// resident stream or what a callback writes into the batch's buffer (the depth file: palace_depth_text_emit).  `stored` (samview -u):
// the members hold stored blocks (DEFLATE BTYPE 00); the device still supplies every CRC, the host only frames the bytes.  `lz`
// (bamsort --lz, samview --lz): the members come from palace_bgzf_deflate_lz, the coder for text without lines.  The EOF member is the
// caller's.
#pragma once
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "bgzf.hpp"
#include "device_scope.hpp"

namespace palace_host {

// laps of a traced run (emit: only with a callback)
struct MemberWriteTimes { double emit = 0, crc = 0, deflate = 0, copy_write = 0; };

// the cut of `bytes` bytes of text into members and batches: no device call in it
inline size_t bgzf_member_count(uint64_t bytes) { return static_cast<size_t>((bytes + kBgzfText - 1) / kBgzfText); }
inline size_t bgzf_batch_members(size_t n_members, size_t batch_cap) { return std::min(batch_cap, std::max<size_t>(1, n_members)); }
struct MemberBatch { size_t nm; uint64_t t_beg, t_end; };
// the batch that begins with member m0: its members' lengths into lens[0 .. nm), its text [t_beg, t_end)
inline MemberBatch bgzf_batch(uint64_t bytes, size_t n_members, size_t batch, size_t m0, int32_t *lens)
{
    MemberBatch b;
    b.nm = std::min(batch, n_members - m0);
    b.t_beg = m0 * kBgzfText;
    b.t_end = std::min<uint64_t>(bytes, (m0 + b.nm) * kBgzfText);
    for (size_t k = 0; k < b.nm; k++) lens[k] = static_cast<int32_t>(std::min<uint64_t>(kBgzfText, b.t_end - (b.t_beg + k * kBgzfText)));
    return b;
}

// one stored member: the 18 bytes of a BGZF header, a final stored block, CRC-32 and ISIZE (len <= kBgzfText, so BSIZE fits)
inline void append_stored_member(std::vector<uint8_t> &out, const uint8_t *data, uint32_t len, uint32_t crc)
{
    const uint32_t bsize = 18 + 5 + len + 8 - 1;
    const uint8_t head[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, static_cast<uint8_t>(bsize), static_cast<uint8_t>(bsize >> 8)};
    out.insert(out.end(), head, head + 18);
    const uint8_t block[5] = {1, static_cast<uint8_t>(len), static_cast<uint8_t>(len >> 8), static_cast<uint8_t>(~len), static_cast<uint8_t>(~len >> 8)};
    out.insert(out.end(), block, block + 5);
    out.insert(out.end(), data, data + len);
    for (uint32_t v : {crc, len})
        for (int k = 0; k < 4; k++) out.push_back(static_cast<uint8_t>(v >> (8 * k)));
}

// where a batch's text comes from: d_stream[t_beg .. t_end) of a resident stream, or fill(t_beg, t_end, d_text) into the batch's buffer
using MemberFill = std::function<void(uint64_t t_beg, uint64_t t_end, uint8_t *d_text)>;

// `bytes` bytes of text to f, members of at most `batch_cap` per batch.  member_off gets every member's file offset, file_bytes grows by
// the bytes written (it is the file offset of the first member on entry).  no_room, write_failed: the caller's messages.
inline void write_members_device(palace_ctx *ctx, NoRoomText no_room, const uint8_t *d_stream, const MemberFill &fill, uint64_t bytes, size_t batch_cap, bool stored,
                                 bool lz, FILE *f, const std::string &write_failed, StageClock &clock, MemberWriteTimes &tm, std::vector<uint64_t> &member_off,
                                 uint64_t &file_bytes)
{
    const size_t n_members = bgzf_member_count(bytes), batch = bgzf_batch_members(n_members, batch_cap);
    if (!n_members) return;
    DeviceScope dev(ctx, no_room);
    const char *what = "a batch of members";
    uint8_t *d_batch_text = fill ? dev.array<uint8_t>(batch * kBgzfText + 16, what) : nullptr;
    uint8_t *d_slots = stored ? nullptr : dev.array<uint8_t>(batch * 65536, what), *d_file = stored ? nullptr : dev.array<uint8_t>(batch * 65536, what);
    std::vector<int64_t> off(batch), moff(batch + 1);
    for (size_t k = 0; k < batch; k++) off[k] = static_cast<int64_t>(k * kBgzfText);
    const int64_t *d_off = dev.upload(off.data(), batch, what);
    int64_t *d_moff = dev.array<int64_t>(batch + 1, what);
    int32_t *d_len = dev.array<int32_t>(batch, what), *d_mlen = dev.array<int32_t>(batch, what);
    uint32_t *d_crc = dev.array<uint32_t>(batch, what);
    std::vector<int32_t> lens(batch);
    std::vector<uint32_t> crc(stored ? batch : 0);
    std::vector<uint8_t> framed;
    PinnedBuffer pinned(ctx, batch * 65536);
    for (size_t m0 = 0; m0 < n_members; m0 += batch) {
        const MemberBatch b = bgzf_batch(bytes, n_members, batch, m0, lens.data());
        const size_t nm = b.nm;
        clock.restart();
        ck(palace_h2d(ctx, d_len, lens.data(), nm * 4), "palace_h2d");
        const uint8_t *d_text = fill ? d_batch_text : d_stream + b.t_beg;
        if (fill) {
            fill(b.t_beg, b.t_end, d_batch_text);
            clock.lap(&tm.emit, true);
        }
        ck(palace_crc32_members(ctx, d_text, static_cast<int64_t>(nm), d_off, d_len, d_crc), "palace_crc32_members");
        clock.lap(&tm.crc, true);
        const uint8_t *bytes_at = static_cast<const uint8_t *>(pinned.p);
        size_t n_bytes;
        if (stored) {
            ck(palace_d2h(ctx, crc.data(), d_crc, nm * 4), "palace_d2h");
            ck(palace_d2h(ctx, pinned.p, d_text, static_cast<size_t>(b.t_end - b.t_beg)), "palace_d2h");
            framed.clear();
            for (size_t k = 0; k < nm; k++) {
                moff[k] = static_cast<int64_t>(framed.size());
                append_stored_member(framed, bytes_at + k * kBgzfText, static_cast<uint32_t>(lens[k]), crc[k]);
            }
            bytes_at = framed.data();
            n_bytes = framed.size();
        } else {
            if (lz) ck(palace_bgzf_deflate_lz(ctx, d_text, static_cast<int64_t>(nm), d_off, d_len, d_crc, d_slots, d_mlen), "palace_bgzf_deflate_lz");
            else ck(palace_bgzf_deflate(ctx, d_text, static_cast<int64_t>(nm), d_off, d_len, d_crc, d_slots, d_mlen), "palace_bgzf_deflate");
            ck(palace_bgzf_compact(ctx, d_slots, static_cast<int64_t>(nm), d_mlen, d_file, d_moff), "palace_bgzf_compact");
            clock.lap(&tm.deflate, true);
            ck(palace_d2h(ctx, moff.data(), d_moff, (nm + 1) * 8), "palace_d2h");
            n_bytes = static_cast<size_t>(moff[nm]);
            ck(palace_d2h(ctx, pinned.p, d_file, n_bytes), "palace_d2h");
        }
        for (size_t k = 0; k < nm; k++) member_off.push_back(file_bytes + static_cast<uint64_t>(moff[k]));
        if (std::fwrite(bytes_at, 1, n_bytes, f) != n_bytes) throw std::runtime_error(write_failed);
        file_bytes += n_bytes;
        clock.lap(&tm.copy_write, true);
    }
}

// the output files of a run: closed, and removed again unless the run came through
struct OutputFiles {
    FILE *f = nullptr;
    std::vector<std::string> made;
    bool done = false;
    ~OutputFiles()
    {
        if (f) std::fclose(f);
        if (!done) for (const std::string &p : made) std::remove(p.c_str());
    }
};

// A BAM stream d_out[0 .. out_bytes) to f as a whole BGZF file (`bamsort`, `samview`): the members, then the 28-byte EOF member; f is left
// open.  member_u / member_c get every member's stream and file offset, the EOF member's last (it stands for the stream's end);
// *file_bytes the bytes written.
inline void write_bam_file_device(palace_ctx *ctx, NoRoomText no_room, const uint8_t *d_out, int64_t out_bytes, size_t batch_cap, bool stored, bool lz, FILE *f,
                                  const std::string &out, StageClock &clock, MemberWriteTimes &tm, std::vector<int64_t> &member_u, std::vector<int64_t> &member_c,
                                  uint64_t *file_bytes)
{
    std::vector<uint64_t> member_off;
    *file_bytes = 0;
    write_members_device(ctx, no_room, d_out, {}, static_cast<uint64_t>(out_bytes), batch_cap, stored, lz, f, "write failed: " + out, clock, tm, member_off, *file_bytes);
    for (size_t k = 0; k < member_off.size(); k++) {
        member_u.push_back(static_cast<int64_t>(k * kBgzfText));
        member_c.push_back(static_cast<int64_t>(member_off[k]));
    }
    member_u.push_back(out_bytes);                                           // the EOF member stands for the stream's end
    member_c.push_back(static_cast<int64_t>(*file_bytes));
    if (std::fwrite(bgzf_eof_member(), 1, 28, f) != 28) throw std::runtime_error("write failed: " + out);
    *file_bytes += 28;
}

}  // namespace palace_host
