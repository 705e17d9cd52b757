// A BAM stream that lies in device memory written as a BGZF file (`bamsort`, `samview`): members of kBgzfText = 0xff00 bytes of stream,
// the last one shorter, a batch at a time -- palace_crc32_members for the trailers, palace_bgzf_deflate and palace_bgzf_compact for
// the members, one copy back per batch (the batch loop of depthgz_device.hpp) -- and the 28-byte EOF member.  `stored` (samview -u):
// the members hold stored blocks (DEFLATE BTYPE 00); the device still supplies every CRC, the host only frames the bytes.
#pragma once
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "bai.hpp"
#include "bgzf.hpp"

namespace palace_host {

// stage clocks of a traced run: lap() waits for the device and adds the time since the last lap to *acc
struct Laps {
    using clk = std::chrono::steady_clock;
    palace_ctx *ctx;
    bool on;
    clk::time_point t0 = clk::now();
    double keys = 0, sort = 0, gather = 0, deflate = 0, copy_write = 0, index = 0;
    void restart() { t0 = clk::now(); }
    void lap(double *acc)
    {
        if (!on) return;
        if (palace_sync(ctx)) throw std::runtime_error(std::string("palace_sync: ") + palace_last_error());
        const auto t1 = clk::now();
        *acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

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

// The stream d_out[0 .. out_bytes) to f, members of at most `batch_cap` per batch, and the EOF member; f is left open.  member_u /
// member_c get every member's stream and file offset, the EOF member's last (it stands for the stream's end); *file_bytes the bytes
// written.  laps: deflate and copy_write.
inline void write_members_device(palace_ctx *ctx, const uint8_t *d_out, int64_t out_bytes, size_t batch_cap, bool stored, FILE *f, const std::string &out,
                                 Laps &laps, std::vector<int64_t> &member_u, std::vector<int64_t> &member_c, uint64_t *file_bytes_out)
{
    auto ck = [](int rc, const char *what) { if (rc) throw std::runtime_error(std::string(what) + ": " + palace_last_error()); };
    const size_t n_members = (static_cast<size_t>(out_bytes) + kBgzfText - 1) / kBgzfText, batch = std::min(batch_cap, std::max<size_t>(1, n_members));
    uint64_t file_bytes = 0;
    {
        BamsortDevice bd(ctx);
        uint8_t *d_slots = stored ? nullptr : static_cast<uint8_t *>(bd.alloc(batch * 65536, "a batch of members"));
        uint8_t *d_file = stored ? nullptr : static_cast<uint8_t *>(bd.alloc(batch * 65536, "a batch of members"));
        int64_t *d_off = bd.array<int64_t>(batch, "a batch of members"), *d_moff = bd.array<int64_t>(batch + 1, "a batch of members");
        int32_t *d_len = bd.array<int32_t>(batch, "a batch of members"), *d_mlen = bd.array<int32_t>(batch, "a batch of members");
        uint32_t *d_crc = bd.array<uint32_t>(batch, "a batch of members");
        std::vector<int64_t> off(batch), moff(batch + 1);
        std::vector<int32_t> lens(batch);
        std::vector<uint32_t> crc(stored ? batch : 0);
        std::vector<uint8_t> framed;
        for (size_t k = 0; k < batch; k++) off[k] = static_cast<int64_t>(k * kBgzfText);
        ck(palace_h2d(ctx, d_off, off.data(), batch * 8), "palace_h2d");
        void *h_file = nullptr;
        ck(palace_host_alloc(ctx, batch * 65536, &h_file), "palace_host_alloc");
        struct Pinned { palace_ctx *ctx; void *p; ~Pinned() { palace_host_free(ctx, p); } } pinned{ctx, h_file};
        for (size_t m0 = 0; m0 < n_members; m0 += batch) {
            const size_t nm = std::min(batch, n_members - m0);
            const uint64_t t_beg = m0 * kBgzfText, t_end = std::min<uint64_t>(static_cast<uint64_t>(out_bytes), (m0 + nm) * kBgzfText);
            for (size_t k = 0; k < nm; k++) lens[k] = static_cast<int32_t>(std::min<uint64_t>(kBgzfText, t_end - (t_beg + k * kBgzfText)));
            laps.restart();
            ck(palace_h2d(ctx, d_len, lens.data(), nm * 4), "palace_h2d");
            const uint8_t *d_text = d_out + t_beg;
            ck(palace_crc32_members(ctx, d_text, static_cast<int64_t>(nm), d_off, d_len, d_crc), "palace_crc32_members");
            const uint8_t *bytes_at = static_cast<const uint8_t *>(h_file);
            size_t bytes;
            if (stored) {
                laps.lap(&laps.deflate);
                ck(palace_d2h(ctx, crc.data(), d_crc, nm * 4), "palace_d2h");
                ck(palace_d2h(ctx, h_file, d_text, static_cast<size_t>(t_end - t_beg)), "palace_d2h");
                framed.clear();
                for (size_t k = 0; k < nm; k++) {
                    moff[k] = static_cast<int64_t>(framed.size());
                    append_stored_member(framed, bytes_at + k * kBgzfText, static_cast<uint32_t>(lens[k]), crc[k]);
                }
                bytes_at = framed.data();
                bytes = framed.size();
            } else {
                ck(palace_bgzf_deflate(ctx, d_text, static_cast<int64_t>(nm), d_off, d_len, d_crc, d_slots, d_mlen), "palace_bgzf_deflate");
                ck(palace_bgzf_compact(ctx, d_slots, static_cast<int64_t>(nm), d_mlen, d_file, d_moff), "palace_bgzf_compact");
                laps.lap(&laps.deflate);
                ck(palace_d2h(ctx, moff.data(), d_moff, (nm + 1) * 8), "palace_d2h");
                bytes = static_cast<size_t>(moff[nm]);
                ck(palace_d2h(ctx, h_file, d_file, bytes), "palace_d2h");
            }
            for (size_t k = 0; k < nm; k++) {
                member_u.push_back(static_cast<int64_t>((m0 + k) * kBgzfText));
                member_c.push_back(static_cast<int64_t>(file_bytes) + moff[k]);
            }
            if (std::fwrite(bytes_at, 1, bytes, f) != bytes) throw std::runtime_error("write failed: " + out);
            file_bytes += bytes;
            laps.lap(&laps.copy_write);
        }
    }
    member_u.push_back(out_bytes);                                           // the EOF member stands for the stream's end
    member_c.push_back(static_cast<int64_t>(file_bytes));
    if (std::fwrite(bgzf_eof_member(), 1, 28, f) != 28) throw std::runtime_error("write failed: " + out);
    *file_bytes_out = file_bytes + 28;
}

}  // namespace palace_host
