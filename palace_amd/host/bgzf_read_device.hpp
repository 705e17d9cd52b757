// BGZF input on the device, stated once for every loader that keeps the text there (load_bam_stream_device, eref's ingest_bgzf,
// bamdepth's read_depth_bgzf): the member table of one batch, the cut of a file's members into batches, and the reader that turns
// each batch of a mapped file into checked text in device memory -- compressed bytes and table up, palace_bgzf_inflate, the host's
// decoder for what the device refused, palace_crc32_members against every trailer.  It knows no file name and no tool: a member that
// cannot be read is a BgzfMemberFault, and the consumer says it in its own words.  It needs bgzf.hpp, device_scope.hpp and
// include/palace_hip.h.  (The writing side: bgzf_members_device.hpp.  The host loader's helper, a different loop: bam_device.hpp.)
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <exception>
#include <vector>

#include "../../include/palace_hip.h"
#include "bgzf.hpp"
#include "device_scope.hpp"

namespace palace_host {

inline uint32_t le32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

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

// the file offsets of member i: its first header byte (behind the trailer in front of it) and the byte behind its trailer
inline uint64_t bgzf_member_start(const std::vector<BgzfMember> &mem, size_t i) { return i ? mem[i - 1].in_off + mem[i - 1].in_len + 8 : uint64_t{0}; }
inline uint64_t bgzf_member_end(const std::vector<BgzfMember> &mem, size_t i) { return mem[i].in_off + mem[i].in_len + 8; }

// The members of a file cut into batches [cut[k], cut[k + 1]) of batch_members (the last one of what is left; no member: no batch),
// and what the largest batch takes: max_in compressed bytes from the start of its first member through its last trailer, max_out
// inflated bytes.  batch_members >= 1.  No device call.
struct BgzfBatchPlan {
    std::vector<size_t> cut;
    uint64_t max_in = 0, max_out = 0;
    size_t batches() const { return cut.size() - 1; }
};
inline BgzfBatchPlan bgzf_batch_plan(const std::vector<BgzfMember> &mem, size_t batch_members)
{
    BgzfBatchPlan p;
    for (size_t i0 = 0; i0 < mem.size(); i0 += batch_members) {
        const size_t last = std::min(mem.size(), i0 + batch_members) - 1;
        p.cut.push_back(i0);
        p.max_in = std::max(p.max_in, bgzf_member_end(mem, last) - bgzf_member_start(mem, i0));
        p.max_out = std::max(p.max_out, mem[last].out_off + mem[last].out_len - mem[i0].out_off);
    }
    p.cut.push_back(mem.size());
    return p;
}

// A member the reader cannot hand on: refused by the device's decoder and by the host's, or inflated to bytes that are not the ones
// its trailer's CRC-32 was made of.  offset: bgzf_member_start of the member.
struct BgzfMemberFault : std::exception {
    enum Kind { refused, crc } kind;
    uint64_t offset;
    BgzfMemberFault(Kind k, uint64_t o) : kind(k), offset(o) {}
    const char *what() const noexcept override { return kind == refused ? "a BGZF member cannot be inflated" : "CRC-32 mismatch in a BGZF member"; }
};

// A consumer's words: its out-of-room text, its failed device call (ck, or ck_device_error), and what it calls the reader's
// allocations (inflated: the per-batch buffer only).
struct BgzfReadStyle { NoRoomText no_room; void (*check)(int rc, const char *what); const char *compressed, *inflated, *table; };

// One batch, checked, in device memory: members [first, first + n) of the file, bytes [in0, in1) of it, out_bytes of text at d_text.
struct BgzfBatch { size_t k, first, n; uint64_t in0, in1; uint8_t *d_text; int64_t out_bytes; };

// upload / inflate / crc: milliseconds of a timed run (StageClock: an untimed run waits for nothing and counts nothing);
// host_inflated: members the device refused and the host inflated.
struct BgzfReadStats { double upload = 0, inflate = 0, crc = 0; int64_t host_inflated = 0; };

// The reader: every batch of the plan in order, each handed to consume(const BgzfBatch &) once it is checked.  It owns the compressed
// batch, the member table and the host's 64 KiB for a refused member -- and, given no d_stream, one buffer of plan.max_out bytes that
// every batch is inflated into.  Given a d_stream (the caller's, resident, as long as the inflated file), a batch lands at d_stream +
// its first member's out_off.  All of it goes when the reader returns or throws: BgzfMemberFault, DeviceNoRoom with the consumer's
// text, or what style.check throws.  A plan without a batch: no call, no allocation.
template <class Consume>
BgzfReadStats read_bgzf_batches(palace_ctx *ctx, const BgzfReadStyle &style, bool timed, const uint8_t *file, size_t file_size,
                                const std::vector<BgzfMember> &mem, const BgzfBatchPlan &plan, uint8_t *d_stream, Consume &&consume)
{
    BgzfReadStats st;
    if (plan.batches() == 0) return st;
    DeviceScope own(ctx, style.no_room);
    uint8_t *d_in = static_cast<uint8_t *>(own.alloc(static_cast<size_t>(plan.max_in) + 64, style.compressed));
    uint8_t *d_batch = d_stream ? nullptr : static_cast<uint8_t *>(own.alloc(static_cast<size_t>(plan.max_out) + 64, style.inflated));
    MemberTable tab{ctx, static_cast<uint8_t *>(own.alloc(MemberTable::kBytes, style.table))};
    std::vector<uint8_t> host_out(65536);
    StageClock clock{ctx, timed};
    for (size_t k = 0; k < plan.batches(); k++) {
        const size_t i0 = plan.cut[k], n = plan.cut[k + 1] - i0;
        const uint64_t in0 = bgzf_member_start(mem, i0), in1 = bgzf_member_end(mem, i0 + n - 1);
        uint8_t *d_out = d_stream ? d_stream + mem[i0].out_off : d_batch;
        tab.fill(&mem[i0], n, in0);
        const int64_t *out_off = tab.out_off(tab.host.data());
        int32_t *status = tab.status(tab.host.data());
        uint32_t *crc = tab.crc(tab.host.data());
        clock.restart();
        style.check(palace_h2d(ctx, d_in, file + in0, static_cast<size_t>(in1 - in0)), "compressed upload");
        style.check(palace_h2d(ctx, tab.dev, tab.host.data(), tab.up_bytes()), "member table");
        clock.lap(&st.upload, true);
        style.check(tab.inflate(d_in, d_out), "palace_bgzf_inflate");
        style.check(palace_d2h(ctx, status, tab.status(tab.dev), 4 * n), "member status");
        for (size_t j = 0; j < n; j++) {                                     // what the device refused: the host's decoder, zlib behind it
            if (status[j] == 0) continue;
            const BgzfMember &m = mem[i0 + j];
            if (!inflate_member(file, file_size, m, host_out.data())) throw BgzfMemberFault(BgzfMemberFault::refused, bgzf_member_start(mem, i0 + j));
            if (m.out_len) style.check(palace_h2d(ctx, d_out + out_off[j], host_out.data(), m.out_len), "inflated upload");
            st.host_inflated++;
        }
        clock.lap(&st.inflate, true);
        style.check(tab.crc32(d_out), "palace_crc32_members");
        style.check(palace_d2h(ctx, crc, tab.crc(tab.dev), 4 * n), "member CRC");
        for (size_t j = 0; j < n; j++)
            if (crc[j] != le32(file + mem[i0 + j].in_off + mem[i0 + j].in_len)) throw BgzfMemberFault(BgzfMemberFault::crc, bgzf_member_start(mem, i0 + j));
        clock.lap(&st.crc, true);
        consume(BgzfBatch{k, i0, n, in0, in1, d_out, out_off[n - 1] + static_cast<int64_t>(mem[i0 + n - 1].out_len)});
    }
    return st;
}

}  // namespace palace_host
