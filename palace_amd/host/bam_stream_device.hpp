// `bamdepth --bam-gpu`: the BAM inflated, walked and decoded on the device -- for the one consumer that
// needs nothing of a record but its match segments.  The file's BGZF members go up a batch at a time (MemberTable, bam_device.hpp),
// palace_bgzf_inflate puts them into ONE device buffer sized from the ISIZE trailers (a member the device decoder refuses:
// inflate_member on the host, its bytes copied up into place, as fastq_gz.hpp does), palace_crc32_members checks every member
// against its trailer, palace_bam_walk finds the records and palace_bam_match_segments leaves the depth stage's (tid, pos, len)
// arrays in device memory.  The header -- magic, l_text, n_ref, names, lengths, the offset of the first record -- is parsed on the
// host from the front members, inflated there.  The alignment records' bytes never cross back.
// What load_bam (bam.cpp) rejects is rejected here, with its message; its behaviour is not touched.  Device memory held at once: the
// inflated stream, one batch of compressed bytes, 8 B per record, 12 B per segment (the stream and the starts are given back once the
// segments are there).  No fall-back: a device error is the caller's error.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/palace_hip.h"
#include "bam_device.hpp"
#include "bgzf.hpp"

namespace palace_host {

struct BamDeviceTimes { double index = 0, header = 0, upload = 0, inflate = 0, crc = 0, walk = 0, segments = 0; };

// members per batch: kMemberBatch; PALACE_OPT_BAM_BATCH=<members> for tests
inline size_t bam_batch_members()
{
    const char *e = std::getenv("PALACE_OPT_BAM_BATCH");
    const long v = e ? std::atol(e) : 0;
    return v > 0 ? static_cast<size_t>(std::min<long>(v, static_cast<long>(kMemberBatch))) : kMemberBatch;
}
// bytes per chunk of the record walk: 0 = the library's default (64 KiB); PALACE_OPT_BAM_CHUNK=<bytes, at least 64> for tests
inline int64_t bam_walk_chunk()
{
    const char *e = std::getenv("PALACE_OPT_BAM_CHUNK");
    const long long v = e ? std::atoll(e) : 0;
    return v > 0 ? std::max<long long>(v, 64) : 0;
}

// thrown when the device cannot hold what the mode keeps there: the message names the way out
struct BamDeviceNoRoom : std::runtime_error { using std::runtime_error::runtime_error; };

// What the depth stage needs of a BAM: the header's targets on the host, the match segments on the device.
struct DeviceBam {
    palace_ctx *ctx = nullptr;
    std::vector<std::string> target_name;
    std::vector<int32_t> target_len;
    int64_t n_records = 0, n_segs = 0, stop = 0, total = 0, first = 0, host_inflated = 0;
    int64_t walk_stats[4] = {0, 0, 0, 0};              // chunks, guesses that held, chunks repaired, chunks without a start
    int32_t *d_tid = nullptr, *d_pos = nullptr, *d_len = nullptr;
    DeviceBam() = default;
    DeviceBam(const DeviceBam &) = delete;
    DeviceBam &operator=(const DeviceBam &) = delete;
    ~DeviceBam() { for (void *p : {static_cast<void *>(d_tid), static_cast<void *>(d_pos), static_cast<void *>(d_len)}) if (p) palace_free(ctx, p); }
};

// Throws std::runtime_error: load_bam's messages for what load_bam rejects, BamDeviceNoRoom, or a device error with
// palace_last_error().  times: every stage waited for (traced runs).
inline void load_bam_device(palace_ctx *ctx, const std::string &path, int threads, DeviceBam &out, BamDeviceTimes *times = nullptr)
{
    using clk = std::chrono::steady_clock;
    auto le32 = [](const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; };
    auto ck = [](int rc, const char *what) { if (rc) throw std::runtime_error(std::string(what) + ": " + palace_last_error()); };
    auto t0 = clk::now();
    BamDeviceTimes unused;
    BamDeviceTimes &tm = times ? *times : unused;
    auto lap = [&](double *acc, bool device) {
        if (!times) return;
        if (device) ck(palace_sync(ctx), "palace_sync");
        const auto t1 = clk::now();
        *acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    };
    out.ctx = ctx;
    std::vector<void *> owned;
    struct Cleanup { palace_ctx *ctx; std::vector<void *> &owned; ~Cleanup() { for (void *p : owned) palace_free(ctx, p); } } cleanup{ctx, owned};
    auto give_back = [&](void *p) { palace_free(ctx, p); owned.erase(std::find(owned.begin(), owned.end(), p)); };
    auto dev = [&](size_t bytes, const char *what) {
        void *p = nullptr;
        if (palace_malloc(ctx, bytes ? bytes : 1, &p))
            throw BamDeviceNoRoom("--bam-gpu keeps the whole inflated BAM on the device and cannot allocate " + std::to_string(bytes) + " bytes for " + what + " (" +
                                  palace_last_error() + "); run without --bam-gpu to load the BAM on the host");
        owned.push_back(p);
        return p;
    };

    // ---- the file and its checked member index ----
    struct Mapped {
        const uint8_t *data = nullptr; size_t size = 0;
        ~Mapped() { if (data) ::munmap(const_cast<uint8_t *>(data), size); }
    } file;
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("Failed to open BAM " + path);
        struct stat st;
        if (::fstat(fd, &st) != 0) { ::close(fd); throw std::runtime_error("Failed to open BAM " + path); }
        file.size = static_cast<size_t>(st.st_size);
        if (file.size) {
            void *m = ::mmap(nullptr, file.size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { ::close(fd); throw std::runtime_error("Failed to read BAM " + path); }
            ::madvise(m, file.size, MADV_SEQUENTIAL);
            file.data = static_cast<const uint8_t *>(m);
        }
        ::close(fd);
    }
    size_t total = 0;
    const std::vector<BgzfMember> mem = bgzf_members(file.data, file.size, &total);
    const size_t nb = mem.size();
    lap(&tm.index, false);

    // ---- the header (BAM spec 4.2), from the front members inflated here: rounds of twice as many members, on the threads ----
    std::vector<uint8_t> hdr;
    size_t hdr_members = 0;
    auto need = [&](size_t upto) {
        while (hdr.size() < upto && hdr_members < nb) {
            const size_t a = hdr_members, b = std::min(nb, a + std::max<size_t>(1, a));
            hdr.resize(static_cast<size_t>(mem[b - 1].out_off + mem[b - 1].out_len));
            std::atomic<size_t> next{a};
            std::atomic<bool> bad{false};
            auto work = [&] {
                for (size_t i; (i = next.fetch_add(1)) < b;)
                    if (!inflate_member(file.data, file.size, mem[i], hdr.data() + mem[i].out_off)) bad = true;
            };
            std::vector<std::thread> pool;
            for (size_t t = 1; t < std::min<size_t>(static_cast<size_t>(std::max(1, threads)), b - a); t++) pool.emplace_back(work);
            work();
            for (auto &th : pool) th.join();
            if (bad) throw std::runtime_error("BGZF inflate failed");
            hdr_members = b;
        }
        if (hdr.size() < upto) throw std::runtime_error("Failed to read BAM header");
    };
    need(12);
    if (std::memcmp(hdr.data(), "BAM\1", 4) != 0) throw std::runtime_error("Failed to read BAM header");
    size_t p = 8 + static_cast<size_t>(le32(hdr.data() + 4));
    need(p + 4);
    const int32_t n_ref = static_cast<int32_t>(le32(hdr.data() + p));
    p += 4;
    for (int32_t i = 0; i < n_ref; i++) {
        need(p + 4);
        const size_t l = le32(hdr.data() + p);
        need(p + 4 + l + 4);
        out.target_name.emplace_back(reinterpret_cast<const char *>(hdr.data() + p + 4), l ? l - 1 : 0);
        out.target_len.push_back(static_cast<int32_t>(le32(hdr.data() + p + 4 + l)));
        p += 8 + l;
    }
    const size_t first = p;
    std::vector<uint8_t>().swap(hdr);
    lap(&tm.header, false);

    // ---- every member inflated into one device buffer, a batch of compressed bytes at a time ----
    const size_t batch = bam_batch_members();
    auto member_start = [&](size_t i) { return i ? mem[i - 1].in_off + mem[i - 1].in_len + 8 : uint64_t{0}; };
    uint64_t max_in = 0;
    for (size_t i0 = 0; i0 < nb; i0 += batch) {
        const size_t i1 = std::min(nb, i0 + batch);
        max_in = std::max<uint64_t>(max_in, mem[i1 - 1].in_off + mem[i1 - 1].in_len + 8 - member_start(i0));
    }
    uint8_t *d_stream = static_cast<uint8_t *>(dev(total + 64, "the inflated stream"));
    if (nb) {
        uint8_t *d_in = static_cast<uint8_t *>(dev(static_cast<size_t>(max_in) + 64, "a batch of compressed bytes"));
        void *d_meta = dev(MemberTable::kBytes, "the member table");
        MemberTable tab{ctx, static_cast<uint8_t *>(d_meta)};
        std::vector<uint8_t> host_out(65536);
        for (size_t i0 = 0; i0 < nb; i0 += batch) {
            const size_t n = std::min(nb, i0 + batch) - i0;
            const uint64_t in0 = member_start(i0), in1 = mem[i0 + n - 1].in_off + mem[i0 + n - 1].in_len + 8;
            uint8_t *d_out = d_stream + mem[i0].out_off;
            tab.fill(&mem[i0], n, in0);
            const int64_t *out_off = tab.out_off(tab.host.data());
            int32_t *status = tab.status(tab.host.data());
            uint32_t *crc = tab.crc(tab.host.data());
            t0 = clk::now();
            ck(palace_h2d(ctx, d_in, file.data + in0, static_cast<size_t>(in1 - in0)), "compressed upload");
            ck(palace_h2d(ctx, d_meta, tab.host.data(), tab.up_bytes()), "member table");
            lap(&tm.upload, true);
            ck(tab.inflate(d_in, d_out), "palace_bgzf_inflate");
            ck(palace_d2h(ctx, status, tab.status(tab.dev), 4 * n), "member status");
            for (size_t j = 0; j < n; j++) {                                 // what the device refused: the host's decoder, zlib behind it
                if (status[j] == 0) continue;
                const BgzfMember &m = mem[i0 + j];
                if (!inflate_member(file.data, file.size, m, host_out.data())) throw std::runtime_error("BGZF inflate failed");
                if (m.out_len) ck(palace_h2d(ctx, d_out + out_off[j], host_out.data(), m.out_len), "inflated upload");
                out.host_inflated++;
            }
            lap(&tm.inflate, true);
            ck(tab.crc32(d_out), "palace_crc32_members");
            ck(palace_d2h(ctx, crc, tab.crc(tab.dev), 4 * n), "member CRC");
            for (size_t j = 0; j < n; j++) {
                const BgzfMember &m = mem[i0 + j];
                if (crc[j] != le32(file.data + m.in_off + m.in_len))
                    throw std::runtime_error("CRC-32 mismatch in the BGZF member at offset " + std::to_string(member_start(i0 + j)));
            }
            lap(&tm.crc, true);
        }
        give_back(d_in);
        give_back(d_meta);
    }

    // ---- the records' starts, then their match segments: each counted first, then written into exactly that much memory ----
    t0 = clk::now();
    const int64_t chunk = bam_walk_chunk();
    const size_t scratch_bytes = palace_bam_walk_scratch_bytes(static_cast<int64_t>(total), static_cast<int64_t>(first), chunk);
    void *d_scratch = dev(scratch_bytes, "the record walk");
    ck(palace_bam_walk(ctx, d_stream, static_cast<int64_t>(total), static_cast<int64_t>(first), n_ref, chunk, d_scratch, scratch_bytes, nullptr, 0,
                       &out.n_records, &out.stop, out.walk_stats), "palace_bam_walk");
    int64_t *d_starts = static_cast<int64_t *>(dev(static_cast<size_t>(out.n_records) * 8, "the record starts"));
    ck(palace_bam_walk_starts(ctx, d_stream, static_cast<int64_t>(total), static_cast<int64_t>(first), chunk, d_scratch, scratch_bytes, d_starts,
                              out.n_records), "palace_bam_walk_starts");
    ck(palace_sync(ctx), "palace_sync");                                    // (the starts are written: the walk's table can go)
    lap(&tm.walk, true);
    give_back(d_scratch);
    ck(palace_bam_match_segments(ctx, d_stream, static_cast<int64_t>(total), d_starts, out.n_records, n_ref, nullptr, nullptr, nullptr, 0, &out.n_segs),
       "palace_bam_match_segments");
    int32_t **seg[3] = {&out.d_tid, &out.d_pos, &out.d_len};
    for (int32_t **s : seg) {
        *s = static_cast<int32_t *>(dev(static_cast<size_t>(out.n_segs) * 4, "the match segments"));
        owned.pop_back();                                                    // (the result's from here on)
    }
    int64_t again = 0;
    ck(palace_bam_match_segments(ctx, d_stream, static_cast<int64_t>(total), d_starts, out.n_records, n_ref, out.d_tid, out.d_pos, out.d_len, out.n_segs,
                                 &again), "palace_bam_match_segments");
    if (again != out.n_segs) throw std::runtime_error("palace_bam_match_segments: two counts of one stream differ");
    ck(palace_sync(ctx), "palace_sync");
    lap(&tm.segments, true);
    out.total = static_cast<int64_t>(total);
    out.first = static_cast<int64_t>(first);
}

}  // namespace palace_host
