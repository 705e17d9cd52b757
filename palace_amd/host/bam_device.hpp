// BGZF members inflated on the device beside the loader's threads (palace_bgzf_inflate: one wavefront per
// member).  The device decodes a whole BAM 2.4 x as fast as sixteen host threads (21 against 8.7 GB/s of
// output) and is idle while generateGraph reads its BAM: a helper thread takes batches of members off the BACK of the file (bam.hpp,
// BackMembers), sends their compressed bytes up, and copies the inflated bytes straight into the loader's stream
// (PALACE_BAM_DEVICE=0: the host alone; see device_inflate_helpers below for what it measured).  A member the
// device decoder refuses goes to the loader's own decoder (zlib behind it), as a member the CPU decoder refuses does.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/palace_hip.h"
#include "bam.hpp"

namespace palace_host {

// Members per launch of palace_bgzf_inflate: a launch takes as long as its slowest member (~20 ms for 64 KiB) however few members it
// has, and the device holds ~7 000 of the decoder's wavefronts at a time (28 per CU).  (eref's FASTQ in batches of one 32 MiB window,
// ~500 members, left it mostly idle: 260 ms against the 1M-contig sample's 2.1 GB of text, 44 ms in batches of 8 192.)
constexpr size_t kMemberBatch = 8192;

// The member table of one batch as palace_bgzf_inflate and palace_crc32_members read it: per member in_off, out_off (int64), in_len,
// out_len, status, crc (int32), one array of n each.  fill() builds it on the host; the caller sends up the first up_bytes() (the
// columns in front of status) in one copy and reads status / crc back.  Offsets are relative to the batch's first input byte (in0)
// and to its first member's output.  inflate() and crc32() return what the palace_* call returns (0: enqueued).
struct MemberTable {
    static constexpr size_t kBytes = 32 * kMemberBatch;                    // a batch's table, host and device
    palace_ctx *ctx;
    uint8_t *dev;                                                          // kBytes of device memory (the caller's)
    std::vector<uint8_t> host = std::vector<uint8_t>(kBytes);
    size_t n = 0;
    void fill(const BgzfMember *m, size_t count, uint64_t in0)
    {
        n = count;
        int64_t *io = in_off(host.data()), *oo = out_off(host.data());
        int32_t *il = in_len(host.data()), *ol = out_len(host.data());
        for (size_t k = 0; k < n; k++) {
            io[k] = static_cast<int64_t>(m[k].in_off - in0); il[k] = static_cast<int32_t>(m[k].in_len);
            oo[k] = static_cast<int64_t>(m[k].out_off - m[0].out_off); ol[k] = static_cast<int32_t>(m[k].out_len);
        }
    }
    size_t up_bytes() const { return 24 * n; }
    // the columns in `base` (host.data() or dev)
    int64_t *in_off(uint8_t *base) const { return reinterpret_cast<int64_t *>(base); }
    int64_t *out_off(uint8_t *base) const { return reinterpret_cast<int64_t *>(base + 8 * n); }
    int32_t *in_len(uint8_t *base) const { return reinterpret_cast<int32_t *>(base + 16 * n); }
    int32_t *out_len(uint8_t *base) const { return reinterpret_cast<int32_t *>(base + 20 * n); }
    int32_t *status(uint8_t *base) const { return reinterpret_cast<int32_t *>(base + 24 * n); }
    uint32_t *crc(uint8_t *base) const { return reinterpret_cast<uint32_t *>(base + 28 * n); }
    // the batch's compressed bytes (d_in = input byte in0) inflated into d_out; status 0: the member's bytes are there
    int inflate(const uint8_t *d_in, uint8_t *d_out) const
    {
        return palace_bgzf_inflate(ctx, d_in, static_cast<int64_t>(n), in_off(dev), in_len(dev), out_off(dev), out_len(dev), d_out, status(dev));
    }
    // crc: the CRC-32 of every member's bytes in d_out
    int crc32(const uint8_t *d_out) const { return palace_crc32_members(ctx, d_out, static_cast<int64_t>(n), out_off(dev), out_len(dev), crc(dev)); }
};

constexpr double kDeviceBatchDeadlineS = 20.0;          // a batch takes ~0.1 s; behind this the device is taken to be hung

inline MemberHelper device_inflate_helper(int device)
{
    return [device](BackMembers &bm) {
        using Clock = std::chrono::steady_clock;
        const auto t_start = Clock::now();
        palace_ctx *ctx = nullptr;
        if (palace_ctx_create(device, &ctx)) return;                           // no device: everything stays with the loader's threads
        void *d_in = nullptr, *d_out = nullptr, *d_meta = nullptr;
        size_t in_cap = 0, out_cap = 0;                                        // sized by the batches claimed, not by the largest batch there could be
        bool up = !palace_malloc(ctx, MemberTable::kBytes, &d_meta);
        MemberTable tab{ctx, static_cast<uint8_t *>(d_meta)};
        auto room = [&](void *&p, size_t &cap, size_t need) {
            if (need + 64 <= cap) return true;
            if (p) palace_free(ctx, p);
            p = nullptr; cap = 0;
            if (palace_malloc(ctx, need + need / 8 + 64, &p)) return false;
            cap = need + need / 8 + 64;
            return true;
        };
        size_t first = 0, n = 0;
        const bool trace = std::getenv("PALACE_TRACE") != nullptr;          // (laps need a sync per phase: traced runs only)
        auto ms_since = [](Clock::time_point a) { return std::chrono::duration<double, std::milli>(Clock::now() - a).count(); };
        double t_up = 0, t_kernel = 0, t_down = 0, t_ready = ms_since(t_start);
        size_t batches = 0, members = 0;
        (void)t_ready;
        while (up && bm.claim(kMemberBatch, &first, &n)) {
            const BgzfMember &a = bm.members[first], &z = bm.members[first + n - 1];
            const uint64_t in0 = a.in_off, in1 = z.in_off + z.in_len, out0 = a.out_off, out1 = z.out_off + z.out_len;
            bool ok = room(d_in, in_cap, static_cast<size_t>(in1 - in0)) && room(d_out, out_cap, static_cast<size_t>(out1 - out0));
            tab.fill(&a, n, in0);
            int32_t *status = tab.status(tab.host.data());
            auto t0 = Clock::now();
            ok = ok && !palace_h2d_async(ctx, d_in, bm.file_data + in0, static_cast<size_t>(in1 - in0)) && !palace_h2d_async(ctx, d_meta, tab.host.data(), tab.up_bytes());
            if (trace) { palace_sync(ctx); t_up += ms_since(t0); t0 = Clock::now(); }
            ok = ok && !tab.inflate(static_cast<const uint8_t *>(d_in), static_cast<uint8_t *>(d_out));
            if (trace) { palace_sync(ctx); t_kernel += ms_since(t0); t0 = Clock::now(); }
            ok = ok && !palace_d2h_async(ctx, status, tab.status(tab.dev), 4 * n) && !palace_d2h_async(ctx, bm.out + out0, d_out, static_cast<size_t>(out1 - out0)) &&
                 !palace_mark(ctx, 0);
            if (ok && palace_mark_wait_for(ctx, 0, kDeviceBatchDeadlineS)) {
                // the batch never came back (a kernel or a copy that does not return): its members' bytes may still be written behind
                // our back, so nothing of this process can be trusted to finish -- say so and leave, instead of letting the loader's
                // walker and decode threads wait for done[] forever
                std::fprintf(stderr, "generateGraph: the device did not return a batch of BGZF members within %.0f s (%s); "
                                     "run with PALACE_BAM_DEVICE=0 to inflate on the host alone\n", kDeviceBatchDeadlineS, palace_last_error());
                std::fflush(stderr);
                std::_Exit(1);
            }
            if (trace) { t_down += ms_since(t0); batches++; members += n; }
            for (size_t k = 0; k < n; k++) bm.finished(first + k, ok && status[k] == 0);
            if (!ok) break;                                                    // the device is out of the game; what is left goes to the threads
        }
        if (trace)
            std::fprintf(stderr, "[bam/device] ready at %.1f ms; %zu batches, %zu members: up %.1f ms, kernel %.1f ms, down %.1f ms; left at %.1f ms\n",
                         t_ready, batches, members, t_up, t_kernel, t_down, ms_since(t_start));
        palace_free(ctx, d_in); palace_free(ctx, d_out); palace_free(ctx, d_meta);
        palace_ctx_destroy(ctx);
    };
}

// the helpers generateGraph starts: PALACE_BAM_DEVICE=<n> helper threads (default 2: one's copies overlap the other's kernel; 0 = the
// host alone).  Measured on the 1M-contig sample's BAM (30 590 members; tools/archive/r04ze.sh, settings alternated on one box): a helper is
// ready 80-100 ms into the run and takes one batch of 3 500-8 000 members (up 25-50 ms, kernel 40-65, down 35-70: the copies through
// pageable memory are the larger part), 11 000 members (38 %) are the device's by the time the sixteen threads have met them from the
// front; generateGraph 0.73 -> 0.68 s, with stage 04 in the process 0.86 -> 0.81 s.  (With the first version of the kernel -- window in
// LDS, four waves per CU, 350 ms for the file -- the helpers got 20 % of the members and the wall time did not move.)
inline std::vector<MemberHelper> device_inflate_helpers(int device)
{
    int n = 2;
    if (const char *e = std::getenv("PALACE_BAM_DEVICE")) n = std::max(0, std::min(4, std::atoi(e)));
    return std::vector<MemberHelper>(static_cast<size_t>(n), device_inflate_helper(device));
}

}  // namespace palace_host
