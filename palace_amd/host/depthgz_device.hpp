// `bamdepth --depth-gz-gpu <out.gz> <bam>`: the files of depthgz.hpp -- <out.gz> (the text of `samtools depth`, BGZF) and
// <out.gz>.tbi -- with the text, its CRC-32, DEFLATE and the index's offsets computed on the device:
//     palace_depth_text_create          depths of every position, where every line of the text lies
//     per batch of members:  palace_depth_text_emit -> palace_crc32_members -> palace_bgzf_deflate -> palace_bgzf_compact,
//                            one copy of the batch's file bytes to the host, fwrite (write_members_device, bgzf_members_device.hpp)
//     palace_depth_text_windows         per contig and 16 kb window: first line's text offset, lines
// The text, the cut into members of 0xff00 bytes, the contig order and the index (virtual offsets mapped back to text offsets) are
// those of the host mode; the DEFLATE bytes are the device coder's (valid, deterministic, not zlib's).  No fall-back: a device
// error is the caller's error.
#pragma once
#include <cstdlib>

#include "bgzf_members_device.hpp"
#include "depthgz.hpp"

namespace palace_host {

struct DepthGzDeviceTimes { double upload = 0, create = 0, windows = 0, tbi = 0; MemberWriteTimes members; };

// members per batch: 8192 (the inflate side's batch: 510 MiB of text, 512 MiB of slots); PALACE_OPT_DEPTHGZ_BATCH=<members> for tests
inline size_t depthgz_batch_members()
{
    const char *e = std::getenv("PALACE_OPT_DEPTHGZ_BATCH");
    const long v = e ? std::atol(e) : 0;
    return v > 0 ? static_cast<size_t>(std::min<long>(v, 8192)) : 8192;
}

// Throws std::runtime_error (with palace_last_error() for a device error).  times: each stage waited for (PALACE_DEPTHGZ_TIMES=1).
// The match segments (ns of them) are in device memory already.
inline DepthGzResult write_depth_gz_device(palace_ctx *ctx, int64_t n_segs, const int32_t *d_tid, const int32_t *d_pos, const int32_t *d_len,
                                           const std::vector<std::string> &target_name, const std::vector<int32_t> &target_len, const std::string &gz_path,
                                           DepthGzDeviceTimes *times = nullptr)
{
    DepthGzDeviceTimes unused;
    DepthGzDeviceTimes &tm = times ? *times : unused;
    StageClock clock{ctx, times != nullptr};
    DeviceScope dev(ctx);
    DepthTextHandle dt(ctx);                                               // (goes before the arrays it was made from)

    const size_t nt = target_len.size(), ns = static_cast<size_t>(n_segs);
    std::vector<int64_t> base(nt + 1, 0);
    for (size_t t = 0; t < nt; t++) base[t + 1] = base[t] + std::max(0, target_len[t]);
    clock.restart();
    const int32_t *d_tlen = dev.upload(target_len.data(), nt, "the contig lengths");
    const int64_t *d_base = dev.upload(base.data(), nt + 1, "the contig bases");
    const DeviceNames names = upload_names(dev, target_name, "the contig names", "palace_h2d");
    clock.lap(&tm.upload, true);
    DepthGzResult res;
    uint64_t text_bytes = 0;
    ck(palace_depth_text_create(ctx, static_cast<int64_t>(ns), d_tid, d_pos, d_len, static_cast<int32_t>(nt), d_tlen, d_base, base[nt], names.blob, names.off,
                                &dt.h, &text_bytes, &res.lines, &res.sum), "palace_depth_text_create");
    clock.lap(&tm.create, true);

    // the file: BgzfTextWriter keeps the member table that write_tbi maps text offsets through; the members come from the device
    BgzfTextWriter w(gz_path, 6, 1);
    write_members_device(ctx, no_room_plain, nullptr,
                         [&](uint64_t t_beg, uint64_t t_end, uint8_t *d_text) { ck(palace_depth_text_emit(ctx, dt.h, t_beg, t_end, d_text), "palace_depth_text_emit"); },
                         text_bytes, depthgz_batch_members(), false, false, w.f, "write failed", clock, tm.members, w.member_off, w.file_bytes);
    w.text_bytes = text_bytes;
    w.close();                                                             // (nothing pending: the EOF member)
    res.text_bytes = w.text_bytes; res.file_bytes = w.file_bytes;

    // the index: one range per contig and 16 kb window
    clock.restart();
    std::vector<int64_t> wb, we;
    std::vector<size_t> first_win(nt + 1, 0);
    for (size_t t = 0; t < nt; t++) {
        const int64_t L = std::max(0, target_len[t]);
        for (int64_t p = 0; p < L; p += 16384) { wb.push_back(base[t] + p); we.push_back(base[t] + std::min(L, p + 16384)); }
        first_win[t + 1] = wb.size();
    }
    const size_t nw = wb.size();
    std::vector<uint64_t> tb(nw), te(nw), nl(nw);
    if (nw && res.lines) {
        const int64_t *d_wb = dev.upload(wb.data(), nw, "the windows"), *d_we = dev.upload(we.data(), nw, "the windows");
        uint64_t *d_tb = dev.array<uint64_t>(nw, "the windows"), *d_te = dev.array<uint64_t>(nw, "the windows"), *d_nl = dev.array<uint64_t>(nw, "the windows");
        ck(palace_depth_text_windows(ctx, dt.h, static_cast<int64_t>(nw), d_wb, d_we, d_tb, d_te, d_nl), "palace_depth_text_windows");
        ck(palace_d2h(ctx, tb.data(), d_tb, nw * 8), "palace_d2h");
        ck(palace_d2h(ctx, te.data(), d_te, nw * 8), "palace_d2h");
        ck(palace_d2h(ctx, nl.data(), d_nl, nw * 8), "palace_d2h");
    }
    clock.lap(&tm.windows, true);
    std::vector<TbiRef> refs;
    for (size_t t = 0; t < nt && res.lines; t++) {
        TbiRef r;
        for (size_t k = first_win[t]; k < first_win[t + 1]; k++) {
            if (!nl[k]) continue;
            const uint32_t win = static_cast<uint32_t>(k - first_win[t]);
            if (r.bins.empty()) r.off_beg = tb[k];
            r.bins.push_back(TbiBin{4681u + win, tb[k], te[k]});
            r.off_end = te[k];
            r.n_lines += nl[k];
            // (an empty window's first-line-at-or-behind is the next covered window's first line: what the linear index wants there)
            while (r.ioff.size() <= win) r.ioff.push_back(tb[first_win[t] + r.ioff.size()]);
        }
        if (r.bins.empty()) continue;
        r.name = target_name[t];
        refs.push_back(std::move(r));
    }
    write_tbi(gz_path + ".tbi", refs, w);
    clock.lap(&tm.tbi, true);
    return res;
}

// the same from the match segments the host loader collected: uploaded, then as above
inline DepthGzResult write_depth_gz_device(palace_ctx *ctx, const BamColumns &c, const std::string &gz_path, DepthGzDeviceTimes *times = nullptr)
{
    const size_t ns = c.mseg_tid.size();
    StageClock clock{ctx, times != nullptr};
    DeviceScope dev(ctx);
    const int32_t *seg[3] = {dev.upload(c.mseg_tid.data(), ns, "the match segments"), dev.upload(c.mseg_pos.data(), ns, "the match segments"),
                             dev.upload(c.mseg_len.data(), ns, "the match segments")};
    if (times) clock.lap(&times->upload, true);
    return write_depth_gz_device(ctx, static_cast<int64_t>(ns), seg[0], seg[1], seg[2], c.target_name, c.target_len, gz_path, times);
}

}  // namespace palace_host
