// `bamdepth --bam-gpu`: the BAM inflated, walked and decoded on the device -- for the one consumer that
// needs nothing of a record but its match segments.  The file's BGZF members go through the batch reader of bgzf_read_device.hpp
// (inflated and CRC-checked on the device, a batch at a time) into ONE device buffer sized from the ISIZE trailers,
// palace_bam_walk finds the records and palace_bam_match_segments leaves the depth stage's (tid, pos, len)
// arrays in device memory.  The header -- magic, l_text, n_ref, names, lengths, the offset of the first record -- is parsed on the
// host from the front members, inflated there.  The alignment records' bytes never cross back.
// What load_bam (bam.cpp) rejects is rejected here, with its message; its behaviour is not touched.  Device memory held at once: the
// inflated stream, one batch of compressed bytes, 8 B per record, 12 B per segment (the stream and the starts are given back once the
// segments are there).  No fall-back: a device error is the caller's error.
// `generateGraph --bam-gpu` uses the same stream part (load_bam_stream_device: everything up to the record starts) and keeps the stream
// and the starts alive for palace_bam_columns / palace_bam_sa_items and its read-name guard (generate_graph_main.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/palace_hip.h"
#include "bgzf_read_device.hpp"
#include "device_scope.hpp"
#include "mapped_file.hpp"

namespace palace_host {

struct BamDeviceTimes { double index = 0, header = 0, upload = 0, inflate = 0, crc = 0, walk = 0, segments = 0, columns = 0, sa = 0; };

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

// the out-of-room text of the --bam-gpu modes: it names the way out
inline std::string bam_gpu_no_room(size_t bytes, const char *what, const char *err)
{
    return "--bam-gpu keeps the whole inflated BAM on the device and cannot allocate " + std::to_string(bytes) + " bytes for " + what + " (" + err +
           "); run without --bam-gpu to load the BAM on the host";
}

// What every reader of a BAM on the device knows of it: the header's targets and the numbers of the stream and its walk.
struct BamStreamInfo {
    std::vector<std::string> target_name;
    std::vector<int32_t> target_len;
    int32_t n_ref = 0;
    int64_t n_records = 0, stop = 0, total = 0, first = 0, host_inflated = 0;
    int64_t walk_stats[4] = {0, 0, 0, 0};              // chunks, guesses that held, chunks repaired, chunks without a start
};

// The part every --bam-gpu mode shares: the inflated, CRC-checked stream and the record starts on the device, alive as long as this
// object is.
struct DeviceBamStream : BamStreamInfo {
    palace_ctx *ctx = nullptr;
    uint8_t *d_stream = nullptr;
    int64_t *d_starts = nullptr;
    DeviceBamStream() = default;
    DeviceBamStream(const DeviceBamStream &) = delete;
    DeviceBamStream &operator=(const DeviceBamStream &) = delete;
    void release()
    {
        for (void *p : {static_cast<void *>(d_stream), static_cast<void *>(d_starts)}) if (p) palace_free(ctx, p);
        d_stream = nullptr; d_starts = nullptr;
    }
    ~DeviceBamStream() { release(); }
};

// What the depth stage needs of a BAM: the match segments on the device.
struct DeviceBam : BamStreamInfo {
    palace_ctx *ctx = nullptr;
    int64_t n_segs = 0;
    int32_t *d_tid = nullptr, *d_pos = nullptr, *d_len = nullptr;
    DeviceBam() = default;
    DeviceBam(const DeviceBam &) = delete;
    DeviceBam &operator=(const DeviceBam &) = delete;
    ~DeviceBam() { for (void *p : {static_cast<void *>(d_tid), static_cast<void *>(d_pos), static_cast<void *>(d_len)}) if (p) palace_free(ctx, p); }
};

// The file's checked member table as palace_bgzf_voffsets takes it: stream offset and file offset of every BGZF member, the last entry
// standing for the stream's end (the EOF member; without one, the file's end).
struct BamMemberTable { std::vector<int64_t> u, c; };

// The file map, the member index, the header, the batches with inflate and CRC, and the walk.
// Throws std::runtime_error: load_bam's messages for what load_bam rejects, DeviceNoRoom, or a device error with
// palace_last_error().  times: every stage waited for (traced runs).
// on_header: called once out.target_name / target_len are there, before the first batch goes up (what depends on the names only can
// start beside the rest; it may take the two vectors out of `out`).  members: the file's member table, for a caller who indexes it.
inline void load_bam_stream_device(palace_ctx *ctx, const std::string &path, int threads, DeviceBamStream &out, BamDeviceTimes *times = nullptr,
                                   const std::function<void()> &on_header = {}, BamMemberTable *members = nullptr)
{
    BamDeviceTimes unused;
    BamDeviceTimes &tm = times ? *times : unused;
    StageClock clock{ctx, times != nullptr};
    auto lap = [&](double *acc, bool device) { clock.lap(acc, device); };
    out.ctx = ctx;
    DeviceScope own(ctx, bam_gpu_no_room);
    auto dev = [&](size_t bytes, const char *what) { return own.alloc(bytes, what); };

    // ---- the file and its checked member index ----
    const MappedFile file(path, MapHint::sequential, "Failed to open BAM ", "Failed to read BAM ");
    size_t total = 0;
    BgzfWalkEnd end;
    const std::vector<BgzfMember> mem = bgzf_members(file.bytes(), file.size, &total, &end);
    const size_t nb = mem.size();
    out.total = static_cast<int64_t>(total);
    auto member_start = [&](size_t i) { return bgzf_member_start(mem, i); };
    if (members) {
        for (size_t i = 0; i < nb; i++) {
            members->u.push_back(static_cast<int64_t>(mem[i].out_off));
            members->c.push_back(static_cast<int64_t>(member_start(i)));
        }
        if (mem.empty() || mem.back().out_len != 0) {                        // no EOF member: the file's end stands for the stream's
            members->u.push_back(static_cast<int64_t>(total));
            members->c.push_back(static_cast<int64_t>(end.offset));
        }
    }
    lap(&tm.index, false);

    // ---- the header (BAM spec 4.2), from the front members inflated here: rounds of twice as many members, on the threads ----
    std::vector<uint8_t> hdr;
    size_t hdr_members = 0;
    // a header that cannot be read: a front member whose bytes are not the ones its trailer's CRC-32 was made of says so (checked
    // here only: a header that reads well is checked with every other member, on the device)
    auto unreadable_header = [&]() -> std::runtime_error {
        for (size_t i = 0; i < hdr_members; i++)
            if (static_cast<uint32_t>(::crc32(::crc32(0L, Z_NULL, 0), hdr.data() + mem[i].out_off, static_cast<uInt>(mem[i].out_len))) !=
                le32(file.bytes() + mem[i].in_off + mem[i].in_len))
                return std::runtime_error("CRC-32 mismatch in the BGZF member at offset " + std::to_string(member_start(i)));
        return std::runtime_error("Failed to read BAM header");
    };
    auto need = [&](size_t upto) {
        while (hdr.size() < upto && hdr_members < nb) {
            const size_t a = hdr_members, b = std::min(nb, a + std::max<size_t>(1, a));
            hdr.resize(static_cast<size_t>(mem[b - 1].out_off + mem[b - 1].out_len));
            std::atomic<size_t> next{a};
            std::atomic<bool> bad{false};
            auto work = [&] {
                for (size_t i; (i = next.fetch_add(1)) < b;)
                    if (!inflate_member(file.bytes(), file.size, mem[i], hdr.data() + mem[i].out_off)) bad = true;
            };
            std::vector<std::thread> pool;
            for (size_t t = 1; t < std::min<size_t>(static_cast<size_t>(std::max(1, threads)), b - a); t++) pool.emplace_back(work);
            work();
            for (auto &th : pool) th.join();
            if (bad) throw std::runtime_error("BGZF inflate failed");
            hdr_members = b;
        }
        if (hdr.size() < upto) throw unreadable_header();
    };
    need(12);
    if (std::memcmp(hdr.data(), "BAM\1", 4) != 0) throw unreadable_header();
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
    if (on_header) on_header();

    // ---- every member inflated into one device buffer, a batch of compressed bytes at a time (bgzf_read_device.hpp) ----
    uint8_t *d_stream = static_cast<uint8_t *>(dev(total + 64, "the inflated stream"));
    try {                                                                    // (a batch is where the walk will find it: nothing to do with it here)
        const BgzfReadStats st = read_bgzf_batches(ctx, {bam_gpu_no_room, ck, "a batch of compressed bytes", nullptr, "the member table"}, times != nullptr,
                                                   file.bytes(), file.size, mem, bgzf_batch_plan(mem, bam_batch_members()), d_stream, [](const BgzfBatch &) {});
        tm.upload += st.upload; tm.inflate += st.inflate; tm.crc += st.crc;
        out.host_inflated = st.host_inflated;
    } catch (const BgzfMemberFault &f) {
        if (f.kind == BgzfMemberFault::refused) throw std::runtime_error("BGZF inflate failed");
        throw std::runtime_error("CRC-32 mismatch in the BGZF member at offset " + std::to_string(f.offset));
    }

    // ---- the records' starts: counted first, then written into exactly that much memory ----
    clock.restart();
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
    own.give_back(d_scratch);
    own.keep(d_stream);
    own.keep(d_starts);
    out.d_stream = d_stream;
    out.d_starts = d_starts;
    out.n_ref = n_ref;
    out.total = static_cast<int64_t>(total);
    out.first = static_cast<int64_t>(first);
}

// `bamdepth --bam-gpu`: the stream part, then the match segments -- counted first, then written into exactly that much memory; the
// stream and the starts are given back once the segments are there.
inline void load_bam_device(palace_ctx *ctx, const std::string &path, int threads, DeviceBam &out, BamDeviceTimes *times = nullptr)
{
    BamDeviceTimes unused;
    BamDeviceTimes &tm = times ? *times : unused;
    DeviceBamStream st;
    load_bam_stream_device(ctx, path, threads, st, times);
    StageClock clock{ctx, times != nullptr};
    out.ctx = ctx;
    static_cast<BamStreamInfo &>(out) = std::move(static_cast<BamStreamInfo &>(st));      // (the names move; st's numbers stay readable)
    DeviceScope own(ctx, bam_gpu_no_room);
    ck(palace_bam_match_segments(ctx, st.d_stream, st.total, st.d_starts, st.n_records, st.n_ref, nullptr, nullptr, nullptr, 0, &out.n_segs),
       "palace_bam_match_segments");
    int32_t **seg[3] = {&out.d_tid, &out.d_pos, &out.d_len};
    for (int32_t **s : seg) {
        *s = static_cast<int32_t *>(own.alloc(static_cast<size_t>(out.n_segs) * 4, "the match segments"));
        own.keep(*s);                                                        // (the result's from here on)
    }
    int64_t again = 0;
    ck(palace_bam_match_segments(ctx, st.d_stream, st.total, st.d_starts, st.n_records, st.n_ref, out.d_tid, out.d_pos, out.d_len, out.n_segs, &again),
       "palace_bam_match_segments");
    if (again != out.n_segs) throw std::runtime_error("palace_bam_match_segments: two counts of one stream differ");
    ck(palace_sync(ctx), "palace_sync");
    clock.lap(&tm.segments, true);
}

}  // namespace palace_host
