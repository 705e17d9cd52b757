// bamdepth --from-depth: the depth file read back -- <bam>.depth (plain text) or <bam>.depth.gz (BGZF), told apart by their first
// bytes -- and reduced on the device to what the driver takes from it: the awk number (sum / NR) and the per-contig table
// (DESIGN.md section 8).  The text never comes back to the host.
//   plain: windows of the mapped file go up through two page-locked staging buffers (the copy of window k + 1 into staging runs
//          while the device works on window k) and through palace_depth_parse.
//   BGZF:  the checked member index, then the batch reader of bgzf_read_device.hpp (inflate and CRC-32 on the device, one buffer per
//          batch of members) and palace_depth_parse over the batch's text as one window.
// Per window the host reads back the cursor's first 64 bytes, 24 bytes per run and the runs' names, and merges the runs by name in
// order of first appearance.  Device memory in flight: one batch of compressed bytes, one batch of text (<= 512 MiB), the parser's
// scratch (80 bytes per 4 KiB of window) and the runs and names of one window (grown when a window needs more).
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/palace_hip.h"
#include "bgzf_read_device.hpp"
#include "device_scope.hpp"
#include "fastx.hpp"

namespace palace_host {

struct DepthReadTimes { double index = 0, upload = 0, inflate = 0, crc = 0, parse = 0, merge = 0; };

struct DepthReadResult {
    uint64_t lines = 0, sum = 0;
    std::vector<std::string> name;                  // contigs in order of first appearance
    std::vector<uint64_t> contig_sum, contig_lines;
    uint64_t text_bytes = 0, runs = 0, host_inflated = 0;
};

// tests only: members per batch (PALACE_OPT_DEPTHIN_BATCH) and bytes per plain-text window (PALACE_OPT_DEPTHIN_WINDOW, rounded up to 16)
inline size_t depthin_batch_members()
{
    const char *e = std::getenv("PALACE_OPT_DEPTHIN_BATCH");
    const long v = e ? std::atol(e) : 0;
    return v > 0 ? static_cast<size_t>(std::min<long>(v, static_cast<long>(kMemberBatch))) : kMemberBatch;
}
inline int64_t depthin_window_bytes()
{
    const char *e = std::getenv("PALACE_OPT_DEPTHIN_WINDOW");
    const long long v = e ? std::atoll(e) : 0;
    const int64_t w = v > 0 ? std::min<long long>(v, 1ll << 30) : (64ll << 20);
    return (w + 15) & ~int64_t{15};
}

class DepthReader {
public:
    DepthReader(palace_ctx *ctx, const std::string &path, bool timed) : ctx_(ctx), path_(path), timed_(timed) {}
    ~DepthReader()
    {
        for (void *p : {d_cur_, d_scratch_, d_runs_, d_names_}) if (p) palace_free(ctx_, p);
    }
    DepthReader(const DepthReader &) = delete;
    DepthReader &operator=(const DepthReader &) = delete;

    DepthReadResult res;
    DepthReadTimes times;

    void init(int64_t max_window)
    {
        scratch_bytes_ = palace_depth_parse_scratch_bytes(max_window);
        ck(palace_malloc(ctx_, scratch_bytes_, &d_scratch_), "parser scratch");
        ck(palace_malloc(ctx_, sizeof(palace_depth_cursor), &d_cur_), "parser cursor");
        ck(palace_memset(ctx_, d_cur_, 0, sizeof(palace_depth_cursor)), "parser cursor");
        room(1 << 16, 1 << 20);
    }
    // d_text[0 .. n) (16-byte aligned device memory) is the file's next window: parsed, its runs merged into `res`
    void parse(const uint8_t *d_text, int64_t n, bool final_window)
    {
        auto t0 = now();
        for (;;) {
            ck(palace_depth_parse(ctx_, d_text, n, final_window ? 1 : 0, static_cast<palace_depth_cursor *>(d_cur_), static_cast<palace_depth_run *>(d_runs_),
                                  runs_cap_, static_cast<uint8_t *>(d_names_), names_cap_, d_scratch_, scratch_bytes_), "palace_depth_parse");
            Head h;
            ck(palace_d2h(ctx_, &h, d_cur_, sizeof h), "parser cursor");
            if (!h.error) { head_ = h; break; }
            // the window's runs or names did not fit: the cursor is as it was but for the flag and says what the window needs
            if (h.win_runs <= runs_cap_ && h.win_name_bytes <= names_cap_) throw std::runtime_error("the depth parser refused a window that fits");
            room(std::max(h.win_runs, runs_cap_), std::max(h.win_name_bytes, names_cap_));
            ck(palace_h2d(ctx_, d_cur_, &head_, sizeof head_), "parser cursor");
        }
        if (timed_) times.parse += ms_since(t0);
        if (head_.bad_line)
            throw std::runtime_error(path_ + ": line " + std::to_string(head_.bad_line) + ": not `contig<TAB>position<TAB>depth` as samtools depth writes it "
                                     "(1-10 digits, at most 2147483647, at most 4096 bytes)");
        t0 = now();
        const size_t nr = static_cast<size_t>(head_.win_runs), nb = static_cast<size_t>(head_.win_name_bytes);
        runs_.resize(nr); names_.resize(nb);
        if (nr) ck(palace_d2h(ctx_, runs_.data(), d_runs_, nr * sizeof(palace_depth_run)), "runs");
        if (nb) ck(palace_d2h(ctx_, &names_[0], d_names_, nb), "run names");
        for (const palace_depth_run &r : runs_) {
            if (static_cast<size_t>(r.name_off) + r.name_len > nb) throw std::runtime_error("the depth parser returned a run outside its names");
            if (r.lines == 0) continue;
            key_.assign(names_, r.name_off, r.name_len);
            auto it = index_.find(key_);
            size_t at;
            if (it == index_.end()) {
                at = res.name.size();
                index_.emplace(key_, at);
                res.name.push_back(key_); res.contig_sum.push_back(0); res.contig_lines.push_back(0);
            } else at = it->second;
            res.contig_sum[at] += r.sum; res.contig_lines[at] += r.lines;
        }
        res.runs += nr; res.text_bytes += static_cast<uint64_t>(n);
        res.lines = static_cast<uint64_t>(head_.lines); res.sum = head_.sum;
        if (timed_) times.merge += ms_since(t0);
    }
    void ck(int rc, const char *what) { ck_device_error(rc, what); }
    static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
    static double ms_since(std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(now() - t).count(); }
    const std::string &path() const { return path_; }
    bool timed() const { return timed_; }

private:
    struct Head { int64_t lines; uint64_t sum; int64_t bad_line, win_runs, win_name_bytes; int32_t tail_len, tail_buf, error, r0; int64_t r1; };
    static_assert(sizeof(Head) == 64, "the head of palace_depth_cursor");
    void room(int64_t runs, int64_t names)
    {
        if (runs > runs_cap_ || !d_runs_) {
            if (d_runs_) palace_free(ctx_, d_runs_);
            d_runs_ = nullptr;
            ck(palace_malloc(ctx_, static_cast<size_t>(runs) * sizeof(palace_depth_run), &d_runs_), "runs");
            runs_cap_ = runs;
        }
        if (names > names_cap_ || !d_names_) {
            if (d_names_) palace_free(ctx_, d_names_);
            d_names_ = nullptr;
            ck(palace_malloc(ctx_, static_cast<size_t>(names), &d_names_), "run names");
            names_cap_ = names;
        }
    }

    palace_ctx *ctx_;
    std::string path_;
    bool timed_;
    void *d_cur_ = nullptr, *d_scratch_ = nullptr, *d_runs_ = nullptr, *d_names_ = nullptr;
    size_t scratch_bytes_ = 0;
    int64_t runs_cap_ = 0, names_cap_ = 0;
    Head head_{};
    std::vector<palace_depth_run> runs_;
    std::string names_, key_;
    std::unordered_map<std::string, size_t> index_;
};

// ---- plain text -------------------------------------------------------------------------------------------------------------------
inline void read_depth_plain(DepthReader &rd, palace_ctx *ctx, const MappedText &t)
{
    const int64_t W = depthin_window_bytes(), N = static_cast<int64_t>(t.size);
    rd.init(std::min(W, std::max<int64_t>(N, 16)));
    const size_t bytes = static_cast<size_t>(std::min(W, std::max<int64_t>(N, 16)));
    const PinnedBuffer pin0(ctx, bytes, "device error (page-locked staging)"), pin1(ctx, bytes, "device error (page-locked staging)");
    void *const pin[2] = {pin0.p, pin1.p};
    DeviceScope dev(ctx, no_room_device_error);
    void *const d_text[2] = {dev.alloc(bytes + 64, "text window"), dev.alloc(bytes + 64, "text window")};
    int64_t p = 0;
    int b = 0;
    int64_t n = std::min(W, N - p);
    if (n) std::memcpy(pin[b], t.data + p, static_cast<size_t>(n));
    do {
        const auto t0 = DepthReader::now();
        if (n) rd.ck(palace_h2d_async(ctx, d_text[b], pin[b], static_cast<size_t>(n)), "text upload");
        const int64_t next = std::min(W, N - (p + n));
        if (next > 0) std::memcpy(pin[b ^ 1], t.data + p + n, static_cast<size_t>(next));    // while the copy of this window runs
        if (rd.timed()) { rd.ck(palace_sync(ctx), "text upload"); rd.times.upload += DepthReader::ms_since(t0); }
        p += n;
        rd.parse(static_cast<const uint8_t *>(d_text[b]), n, p == N);
        n = next; b ^= 1;
    } while (p < N);
}

// ---- BGZF: inflated, checked and parsed on the device -------------------------------------------------------------------------------
inline void read_depth_bgzf(DepthReader &rd, palace_ctx *ctx, const MappedText &t, const std::vector<BgzfMember> &mem)
{
    const BgzfBatchPlan plan = bgzf_batch_plan(mem, depthin_batch_members());
    rd.init(static_cast<int64_t>(plan.max_out));
    const BgzfReadStyle style{no_room_device_error, ck_device_error, "compressed batch", "inflated batch", "member table"};
    if (mem.empty()) {                                                       // a file without a member: no text
        DeviceScope dev(ctx, style.no_room);
        rd.parse(static_cast<const uint8_t *>(dev.alloc(64, style.inflated)), 0, true);
    }
    try {                                                                    // the batch's text as one window
        const BgzfReadStats st = read_bgzf_batches(ctx, style, rd.timed(), reinterpret_cast<const uint8_t *>(t.data), t.size, mem, plan, nullptr,
                                                   [&](const BgzfBatch &b) { rd.parse(b.d_text, b.out_bytes, b.k + 1 == plan.batches()); });
        rd.times.upload += st.upload; rd.times.inflate += st.inflate; rd.times.crc += st.crc;
        rd.res.host_inflated = static_cast<uint64_t>(st.host_inflated);
    } catch (const BgzfMemberFault &f) {
        if (f.kind == BgzfMemberFault::refused)
            throw std::runtime_error(rd.path() + ": the BGZF member at offset " + std::to_string(f.offset) + " cannot be inflated to the size its trailer states");
        throw std::runtime_error(rd.path() + ": CRC-32 mismatch in the BGZF member at offset " + std::to_string(f.offset));
    }
}

// The depth file `path` read on the device.  Throws std::runtime_error with a message that names the file.
inline DepthReadResult read_depth_file(palace_ctx *ctx, const std::string &path, DepthReadTimes *times)
{
    MappedText t(path);
    DepthReader rd(ctx, path, times != nullptr);
    const uint8_t *d = reinterpret_cast<const uint8_t *>(t.data);
    if (t.size < 2 || d[0] != 0x1f || d[1] != 0x8b) {
        read_depth_plain(rd, ctx, t);
    } else {
        const auto t0 = DepthReader::now();
        std::vector<BgzfMember> mem;
        BgzfWalkEnd end;
        size_t total = 0;
        try {
            mem = bgzf_members(d, t.size, &total, &end);
        } catch (const std::exception &e) {
            if (end.not_bgzf && end.offset == 0)
                throw std::runtime_error(path + ": gzip, but not BGZF (the member at offset " + std::to_string(end.offset) +
                                         " has no BC subfield); only bgzip-compressed depth files are read");
            if (end.not_bgzf)
                throw std::runtime_error(path + ": bytes that are no BGZF member behind the last member, at offset " + std::to_string(end.offset));
            throw std::runtime_error(path + ": truncated or damaged BGZF member at offset " + std::to_string(end.offset) + " (" + e.what() + ")");
        }
        if (end.offset != t.size)
            throw std::runtime_error(path + ": " + std::to_string(t.size - end.offset) + " bytes that are no BGZF member behind the last member, at offset " +
                                     std::to_string(end.offset));
        rd.times.index = DepthReader::ms_since(t0);
        read_depth_bgzf(rd, ctx, t, mem);
    }
    if (times) *times = rd.times;
    return std::move(rd.res);
}

}  // namespace palace_host
