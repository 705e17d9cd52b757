// `bamdepth --depth-gz-gpu <out.gz> <bam>`: the files of depthgz.hpp -- <out.gz> (the text of `samtools depth`, BGZF) and
// <out.gz>.tbi -- with the text, its CRC-32, DEFLATE and the index's offsets computed on the device:
//     palace_depth_text_create          depths of every position, where every line of the text lies
//     per batch of members:  palace_depth_text_emit -> palace_crc32_members -> palace_bgzf_deflate -> palace_bgzf_compact,
//                            one copy of the batch's file bytes to the host, fwrite
//     palace_depth_text_windows         per contig and 16 kb window: first line's text offset, lines
// The text, the cut into members of 0xff00 bytes, the contig order and the index (virtual offsets mapped back to text offsets) are
// those of the host mode; the DEFLATE bytes are the device coder's (valid, deterministic, not zlib's).  No fall-back: a device
// error is the caller's error.
#pragma once
#include <chrono>
#include <cstdlib>

#include "../../include/palace_hip.h"
#include "depthgz.hpp"

namespace palace_host {

struct DepthGzDeviceTimes { double upload = 0, create = 0, emit = 0, crc = 0, deflate = 0, copy_write = 0, windows = 0, tbi = 0; };

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
    using clk = std::chrono::steady_clock;
    auto ck = [](int rc, const char *what) { if (rc) throw std::runtime_error(std::string(what) + ": " + palace_last_error()); };
    auto lap = [&](clk::time_point &t0, double *acc) {
        if (!times) return;
        ck(palace_sync(ctx), "palace_sync");
        const auto t1 = clk::now();
        *acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    };
    std::vector<void *> owned;
    palace_depth_text *dt = nullptr;
    struct Cleanup {
        palace_ctx *ctx; std::vector<void *> &owned; palace_depth_text *&dt;
        ~Cleanup() { palace_depth_text_destroy(ctx, dt); for (void *p : owned) palace_free(ctx, p); }
    } cleanup{ctx, owned, dt};
    auto dev = [&](size_t bytes) { void *p = nullptr; ck(palace_malloc(ctx, bytes ? bytes : 1, &p), "palace_malloc"); owned.push_back(p); return p; };
    auto up = [&](const void *h, size_t bytes) { void *p = dev(bytes); ck(palace_h2d(ctx, p, h, bytes), "palace_h2d"); return p; };

    const size_t nt = target_len.size(), ns = static_cast<size_t>(n_segs);
    std::vector<int64_t> base(nt + 1, 0), name_off(nt + 1, 0);
    std::string names;
    for (size_t t = 0; t < nt; t++) {
        base[t + 1] = base[t] + std::max(0, target_len[t]);
        names += target_name[t];
        name_off[t + 1] = static_cast<int64_t>(names.size());
    }
    auto t0 = clk::now();
    const int32_t *d_tlen = static_cast<const int32_t *>(up(target_len.data(), nt * 4));
    const int64_t *d_base = static_cast<const int64_t *>(up(base.data(), (nt + 1) * 8)), *d_name_off = static_cast<const int64_t *>(up(name_off.data(), (nt + 1) * 8));
    const uint8_t *d_names = static_cast<const uint8_t *>(up(names.data(), names.size()));
    lap(t0, times ? &times->upload : nullptr);
    DepthGzResult res;
    uint64_t text_bytes = 0;
    ck(palace_depth_text_create(ctx, static_cast<int64_t>(ns), d_tid, d_pos, d_len, static_cast<int32_t>(nt), d_tlen, d_base, base[nt], d_names,
                                d_name_off, &dt, &text_bytes, &res.lines, &res.sum), "palace_depth_text_create");
    lap(t0, times ? &times->create : nullptr);

    // the file: BgzfTextWriter keeps the member table that write_tbi maps text offsets through; the members come from the device
    BgzfTextWriter w(gz_path, 6, 1);
    const size_t n_members = static_cast<size_t>((text_bytes + kBgzfText - 1) / kBgzfText), batch = std::min(depthgz_batch_members(), std::max<size_t>(1, n_members));
    if (n_members) {
        uint8_t *d_text = static_cast<uint8_t *>(dev(batch * kBgzfText + 16)), *d_slots = static_cast<uint8_t *>(dev(batch * 65536)),
                *d_file = static_cast<uint8_t *>(dev(batch * 65536));
        std::vector<int64_t> off(batch);
        for (size_t k = 0; k < batch; k++) off[k] = static_cast<int64_t>(k * kBgzfText);
        const int64_t *d_off = static_cast<const int64_t *>(up(off.data(), batch * 8));
        int32_t *d_mlen_in = static_cast<int32_t *>(dev(batch * 4)), *d_mlen = static_cast<int32_t *>(dev(batch * 4));
        uint32_t *d_crc = static_cast<uint32_t *>(dev(batch * 4));
        int64_t *d_moff = static_cast<int64_t *>(dev((batch + 1) * 8));
        std::vector<int32_t> lens(batch);
        std::vector<int64_t> moff(batch + 1);
        void *h_file = nullptr;
        ck(palace_host_alloc(ctx, batch * 65536, &h_file), "palace_host_alloc");
        struct Pinned { palace_ctx *ctx; void *p; ~Pinned() { palace_host_free(ctx, p); } } pinned{ctx, h_file};
        for (size_t m0 = 0; m0 < n_members; m0 += batch) {
            const size_t nm = std::min(batch, n_members - m0);
            const uint64_t t_beg = m0 * kBgzfText, t_end = std::min<uint64_t>(text_bytes, (m0 + nm) * kBgzfText);
            for (size_t k = 0; k < nm; k++) lens[k] = static_cast<int32_t>(std::min<uint64_t>(kBgzfText, t_end - (t_beg + k * kBgzfText)));
            t0 = clk::now();
            ck(palace_h2d(ctx, d_mlen_in, lens.data(), nm * 4), "palace_h2d");
            ck(palace_depth_text_emit(ctx, dt, t_beg, t_end, d_text), "palace_depth_text_emit");
            lap(t0, times ? &times->emit : nullptr);
            ck(palace_crc32_members(ctx, d_text, static_cast<int64_t>(nm), d_off, d_mlen_in, d_crc), "palace_crc32_members");
            lap(t0, times ? &times->crc : nullptr);
            ck(palace_bgzf_deflate(ctx, d_text, static_cast<int64_t>(nm), d_off, d_mlen_in, d_crc, d_slots, d_mlen), "palace_bgzf_deflate");
            ck(palace_bgzf_compact(ctx, d_slots, static_cast<int64_t>(nm), d_mlen, d_file, d_moff), "palace_bgzf_compact");
            lap(t0, times ? &times->deflate : nullptr);
            ck(palace_d2h(ctx, moff.data(), d_moff, (nm + 1) * 8), "palace_d2h");
            const size_t bytes = static_cast<size_t>(moff[nm]);
            ck(palace_d2h(ctx, h_file, d_file, bytes), "palace_d2h");
            for (size_t k = 0; k < nm; k++) w.member_off.push_back(w.file_bytes + static_cast<uint64_t>(moff[k]));
            if (std::fwrite(h_file, 1, bytes, w.f) != bytes) throw std::runtime_error("write failed");
            w.file_bytes += bytes;
            w.text_bytes = t_end;
            lap(t0, times ? &times->copy_write : nullptr);
        }
    }
    w.close();                                                             // (nothing pending: the EOF member)
    res.text_bytes = w.text_bytes; res.file_bytes = w.file_bytes;

    // the index: one range per contig and 16 kb window
    t0 = clk::now();
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
        const int64_t *d_wb = static_cast<const int64_t *>(up(wb.data(), nw * 8)), *d_we = static_cast<const int64_t *>(up(we.data(), nw * 8));
        uint64_t *d_tb = static_cast<uint64_t *>(dev(nw * 8)), *d_te = static_cast<uint64_t *>(dev(nw * 8)), *d_nl = static_cast<uint64_t *>(dev(nw * 8));
        ck(palace_depth_text_windows(ctx, dt, static_cast<int64_t>(nw), d_wb, d_we, d_tb, d_te, d_nl), "palace_depth_text_windows");
        ck(palace_d2h(ctx, tb.data(), d_tb, nw * 8), "palace_d2h");
        ck(palace_d2h(ctx, te.data(), d_te, nw * 8), "palace_d2h");
        ck(palace_d2h(ctx, nl.data(), d_nl, nw * 8), "palace_d2h");
    }
    lap(t0, times ? &times->windows : nullptr);
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
    lap(t0, times ? &times->tbi : nullptr);
    return res;
}

// the same from the match segments the host loader collected: uploaded, then as above
inline DepthGzResult write_depth_gz_device(palace_ctx *ctx, const BamColumns &c, const std::string &gz_path, DepthGzDeviceTimes *times = nullptr)
{
    auto ck = [](int rc, const char *what) { if (rc) throw std::runtime_error(std::string(what) + ": " + palace_last_error()); };
    const size_t ns = c.mseg_tid.size();
    void *seg[3] = {nullptr, nullptr, nullptr};
    struct Cleanup { palace_ctx *ctx; void **seg; ~Cleanup() { for (int k = 0; k < 3; k++) palace_free(ctx, seg[k]); } } cleanup{ctx, seg};
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t *host[3] = {c.mseg_tid.data(), c.mseg_pos.data(), c.mseg_len.data()};
    for (int k = 0; k < 3; k++) {
        ck(palace_malloc(ctx, ns ? ns * 4 : 1, &seg[k]), "palace_malloc");
        ck(palace_h2d(ctx, seg[k], host[k], ns * 4), "palace_h2d");
    }
    if (times) {
        ck(palace_sync(ctx), "palace_sync");
        times->upload += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    return write_depth_gz_device(ctx, static_cast<int64_t>(ns), static_cast<const int32_t *>(seg[0]), static_cast<const int32_t *>(seg[1]),
                                 static_cast<const int32_t *>(seg[2]), c.target_name, c.target_len, gz_path, times);
}

}  // namespace palace_host
