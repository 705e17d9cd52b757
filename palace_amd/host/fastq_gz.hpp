// eref's compressed inputs: a FASTQ file given as gzip (BGZF or any other) becomes part of ONE ASCII read set in HBM -- side 2's
// reads behind side 1's, as the plain path has them -- and is counted from there.
//   BGZF: the batch reader of bgzf_read_device.hpp inflates and CRC-checks the members on the device, a batch at a time, and
//         palace_fastq_parse appends each batch's sequence lines to the read set.  The text never leaves the device.
//   other gzip: palace_gzip_inflate cuts the DEFLATE stream at block starts it finds, inflates the chunks on the device, checks
//         CRC-32 and ISIZE of every member and hands the text to the parser.  What it declines (damaged input, a stream it cannot
//         cut) goes through zlib on a host thread of its own (headers, CRC-32 and ISIZE of every member checked by zlib), the text
//         in chunks through page-locked staging buffers to the device, parsed there by the same kernels: zlib's verdict is the
//         one the user sees.
//   plain (the other side of a mixed pair): the mapped text goes up a window at a time.
// Device memory for text in flight is one window (plus its compressed bytes); host memory for inflated text is the staging ring.
#pragma once
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../include/palace_hip.h"
#include "bgzf_read_device.hpp"
#include "device_scope.hpp"
#include "fastx.hpp"

namespace palace_host {

enum class FqKind { Plain, Bgzf, Gzip };

// By content, not by name: no gzip magic = plain text; gzip whose members the BGZF walker accepts from the first byte to the last
// = BGZF; any other gzip = zlib's (which then also decides what is truncated or trailing).
inline FqKind classify_fastq(const MappedText &t, std::vector<BgzfMember> *members)
{
    const uint8_t *d = reinterpret_cast<const uint8_t *>(t.data);
    if (t.size < 2 || d[0] != 0x1f || d[1] != 0x8b) return FqKind::Plain;
    try {
        size_t total = 0;
        std::vector<BgzfMember> m = bgzf_members(d, t.size, &total);
        if (!m.empty() && m.back().in_off + m.back().in_len + 8 == t.size) { *members = std::move(m); return FqKind::Bgzf; }
    } catch (const std::exception &) {
    }
    return FqKind::Gzip;
}

struct FqIngestTimes { double inflate = 0, crc = 0, parse = 0, h2d = 0; };

// The read set in HBM and the parser's state; grows (device copy) when a window could overrun it.
class DeviceReadSet {
public:
    DeviceReadSet(palace_ctx *ctx, int64_t window, bool timed) : ctx_(ctx), window_(window), timed_(timed) {}
    ~DeviceReadSet() { release_window(); release_set(); }
    DeviceReadSet(const DeviceReadSet &) = delete;
    DeviceReadSet &operator=(const DeviceReadSet &) = delete;

    int64_t window() const { return window_; }
    bool timed() const { return timed_; }
    // forget the reads behind `c` (a cursor() taken earlier): the file they came from is read again
    void rewind(const palace_fastq_cursor &c) { cur_.reads = c.reads; cur_.bases = c.bases; }
    uint8_t *text() const { return d_text_; }
    const palace_fastq_cursor &cursor() const { return cur_; }
    uint8_t *bases() const { return d_bases_; }
    int64_t *offsets() const { return d_offsets_; }
    FqIngestTimes times;

    void init(int64_t bases_guess)
    {
        ck(palace_malloc(ctx_, static_cast<size_t>(window_) + 64, reinterpret_cast<void **>(&d_text_)), "text window");
        scratch_bytes_ = palace_fastq_scratch_bytes(window_);
        ck(palace_malloc(ctx_, scratch_bytes_, &d_scratch_), "parser scratch");
        ck(palace_malloc(ctx_, sizeof(palace_fastq_cursor), reinterpret_cast<void **>(&d_cur_)), "parser cursor");
        grow(std::max<int64_t>(bases_guess, 1 << 20), std::max<int64_t>(bases_guess / 64, 1 << 16));
        const int64_t zero = 0;
        ck(palace_h2d(ctx_, d_offsets_, &zero, 8), "read set");
    }
    // a new file: its first line is line 0, its reads go behind the ones there
    void start_file()
    {
        cur_.line = 0; cur_.open = 0;
        ck(palace_h2d(ctx_, d_cur_, &cur_, sizeof cur_), "parser cursor");
    }
    // d_text_[0 .. n) holds the file's next n bytes (n <= window)
    void parse(int64_t n, bool final_window) { parse_at(d_text_, n, final_window); }
    // ... or another 16-byte aligned device buffer does
    void parse_at(const uint8_t *d_txt, int64_t n, bool final_window)
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (cur_.bases + n > bases_cap_ || cur_.reads + n / 4 + 3 > offsets_cap_)
            grow(std::max(cur_.bases + n, bases_cap_ + bases_cap_ / 2), std::max(cur_.reads + n / 4 + 3, offsets_cap_ + offsets_cap_ / 2));
        ck(palace_fastq_parse(ctx_, d_txt, n, final_window ? 1 : 0, d_cur_, d_bases_, bases_cap_, d_offsets_, offsets_cap_, d_scratch_,
                              scratch_bytes_), "palace_fastq_parse");
        ck(palace_d2h(ctx_, &cur_, d_cur_, sizeof cur_), "parser cursor");
        if (cur_.error) throw std::runtime_error("the FASTQ parser ran out of room");
        if (timed_) times.parse += ms_since(t0);
    }
    void release_window()
    {
        if (d_text_) palace_free(ctx_, d_text_);
        if (d_scratch_) palace_free(ctx_, d_scratch_);
        if (d_cur_) palace_free(ctx_, d_cur_);
        d_text_ = nullptr; d_scratch_ = nullptr; d_cur_ = nullptr;
    }
    void release_set()
    {
        if (d_bases_) palace_free(ctx_, d_bases_);
        if (d_offsets_) palace_free(ctx_, d_offsets_);
        d_bases_ = nullptr; d_offsets_ = nullptr;
    }
    static double ms_since(std::chrono::steady_clock::time_point t)
    {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
    void ck(int rc, const char *what) { ck_device_error(rc, what); }

private:
    void grow(int64_t bases_cap, int64_t offsets_cap)
    {
        void *b = nullptr, *o = nullptr;
        ck(palace_malloc(ctx_, static_cast<size_t>(bases_cap) + 64, &b), "read set");
        ck(palace_malloc(ctx_, static_cast<size_t>(offsets_cap) * 8, &o), "read set");
        if (d_bases_) {
            if (cur_.bases) ck(palace_d2d(ctx_, b, d_bases_, static_cast<size_t>(cur_.bases)), "read set");
            ck(palace_d2d(ctx_, o, d_offsets_, static_cast<size_t>(cur_.reads + 1) * 8), "read set");
            ck(palace_sync(ctx_), "read set");
            release_set();
        }
        d_bases_ = static_cast<uint8_t *>(b); d_offsets_ = static_cast<int64_t *>(o);
        bases_cap_ = bases_cap; offsets_cap_ = offsets_cap;
    }

    palace_ctx *ctx_;
    int64_t window_;
    bool timed_;
    uint8_t *d_text_ = nullptr, *d_bases_ = nullptr;
    int64_t *d_offsets_ = nullptr;
    void *d_scratch_ = nullptr;
    size_t scratch_bytes_ = 0;
    palace_fastq_cursor *d_cur_ = nullptr;
    palace_fastq_cursor cur_{0, 0, 0, 0, 0};
    int64_t bases_cap_ = 0, offsets_cap_ = 0;
};

// ---- plain text (one side of a mixed pair) ---------------------------------------------------------------------------------
inline void ingest_plain(DeviceReadSet &rs, palace_ctx *ctx, const MappedText &t)
{
    rs.start_file();
    const int64_t W = rs.window(), N = static_cast<int64_t>(t.size);
    int64_t p = 0;
    do {
        const int64_t n = std::min(W, N - p);
        const auto t0 = std::chrono::steady_clock::now();
        if (n) rs.ck(palace_h2d(ctx, rs.text(), t.data + p, static_cast<size_t>(n)), "text upload");
        rs.times.h2d += DeviceReadSet::ms_since(t0);
        p += n;
        rs.parse(n, p == N);
    } while (p < N);
}

// ---- BGZF: inflated, checked and parsed on the device ------------------------------------------------------------------------
inline void ingest_bgzf(DeviceReadSet &rs, palace_ctx *ctx, const MappedText &t, const std::vector<BgzfMember> &mem, const std::string &path)
{
    rs.start_file();
    const int64_t W = rs.window();
    // Members are inflated and checked kMemberBatch at a time (bgzf_read_device.hpp); the parser takes a batch's text a window at a
    // time.  Device memory: <= kMemberBatch x 64 KiB of text.
    const BgzfReadStyle style{no_room_device_error, ck_device_error, "compressed window", "inflated window", "member table"};
    try {
        const BgzfReadStats st = read_bgzf_batches(ctx, style, rs.timed(), reinterpret_cast<const uint8_t *>(t.data), t.size, mem,
                                                   bgzf_batch_plan(mem, kMemberBatch), nullptr, [&](const BgzfBatch &b) {
            // The file's last line is closed by the batch that ends with the file's last byte.  (classify_fastq takes a file as BGZF
            // only when its last member ends there, so today this is the last batch; a caller that let stray bytes follow the last
            // member would never see its last line closed through this flag.)
            const bool last_batch = b.in1 == t.size;
            int64_t p = 0;
            do {                                                             // (windows start 16-byte aligned: W is a multiple of 16)
                const int64_t w = std::min(W, b.out_bytes - p);
                rs.parse_at(b.d_text + p, w, last_batch && p + w == b.out_bytes);
                p += w;
            } while (p < b.out_bytes);
        });
        rs.times.h2d += st.upload; rs.times.inflate += st.inflate; rs.times.crc += st.crc;
    } catch (const BgzfMemberFault &f) {
        if (f.kind == BgzfMemberFault::refused) throw std::runtime_error(path + ": the BGZF member at offset " + std::to_string(f.offset) + " cannot be inflated");
        throw std::runtime_error(path + ": CRC-32 mismatch in the BGZF member at offset " + std::to_string(f.offset));
    }
}

// ---- other gzip: zlib on a thread of its own, text through a ring of page-locked buffers -------------------------------------
class GzipProducer {
public:
    GzipProducer(palace_ctx *ctx, const MappedText &t, const std::string &path, int64_t chunk) : t_(t), path_(path), chunk_(chunk)
    {
        for (int k = 0; k < kRing; k++) {
            void *p = nullptr;
            if (palace_host_alloc(ctx, static_cast<size_t>(chunk_), &p)) throw std::runtime_error(std::string("cannot page-lock staging: ") + palace_last_error());
            buf_[k] = static_cast<uint8_t *>(p);
        }
        ctx_ = ctx;
        th_ = std::thread([this] { run(); });
    }
    ~GzipProducer()
    {
        {
            std::lock_guard<std::mutex> g(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        if (th_.joinable()) th_.join();
        for (int k = 0; k < kRing; k++) palace_host_free(ctx_, buf_[k]);
    }
    // the next chunk: bytes in *n (0 and true = the end); throws what the inflater found
    const uint8_t *next(int64_t *n, bool *last)
    {
        std::unique_lock<std::mutex> g(mu_);
        if (taken_) { taken_ = false; head_++; cv_.notify_all(); }          // the previous chunk is free again
        cv_.wait(g, [&] { return tail_ > head_ || done_; });
        if (tail_ > head_) {
            *n = len_[head_ % kRing];
            *last = done_ && tail_ == head_ + 1 && err_.empty();
            taken_ = true;
            return buf_[head_ % kRing];
        }
        if (!err_.empty()) throw std::runtime_error(err_);
        *n = 0; *last = true;
        return nullptr;
    }
    double inflate_ms() const { return inflate_ms_; }

private:
    static constexpr int kRing = 3;
    void fail(const std::string &m)
    {
        std::lock_guard<std::mutex> g(mu_);
        err_ = path_ + ": " + m;
        done_ = true;
        cv_.notify_all();
    }
    void run()
    {
        const auto t0 = std::chrono::steady_clock::now();
        z_stream zs{};
        if (inflateInit2(&zs, 15 + 16) != Z_OK) { fail("zlib cannot start"); return; }
        const uint8_t *in = reinterpret_cast<const uint8_t *>(t_.data);
        size_t pos = 0;
        bool in_member = false;
        std::string err;
        for (;;) {
            uint8_t *dst;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return tail_ - head_ < kRing || stop_; });
                if (stop_) break;
                dst = buf_[tail_ % kRing];
            }
            int64_t filled = 0;
            bool end = false;
            while (filled < chunk_ && err.empty()) {
                if (!in_member) {
                    if (pos == t_.size) { end = true; break; }
                    if (t_.size - pos < 2 || in[pos] != 0x1f || in[pos + 1] != 0x8b) {
                        err = pos ? "bytes that are not gzip after the last member (offset " + std::to_string(pos) + ")" : "not a gzip file";
                        break;
                    }
                    if (inflateReset(&zs) != Z_OK) { err = "zlib cannot restart"; break; }
                    in_member = true;
                }
                const size_t avail = std::min<size_t>(t_.size - pos, 1u << 30);
                zs.next_in = const_cast<Bytef *>(in + pos); zs.avail_in = static_cast<uInt>(avail);
                zs.next_out = dst + filled; zs.avail_out = static_cast<uInt>(chunk_ - filled);
                const int rc = inflate(&zs, Z_NO_FLUSH);
                pos += avail - zs.avail_in;
                filled = chunk_ - zs.avail_out;
                if (rc == Z_STREAM_END) { in_member = false; continue; }     // CRC-32 and ISIZE checked by zlib
                if (rc == Z_OK) continue;
                if (rc == Z_BUF_ERROR && zs.avail_out == 0) continue;
                if (rc == Z_BUF_ERROR) { err = "truncated gzip stream"; break; }
                err = std::string("corrupt gzip stream (") + (zs.msg ? zs.msg : "zlib error") + ") near offset " + std::to_string(pos);
                break;
            }
            {
                std::lock_guard<std::mutex> g(mu_);
                if (filled) { len_[tail_ % kRing] = filled; tail_++; }
                if (!err.empty()) { err_ = path_ + ": " + err; done_ = true; }
                else if (end) done_ = true;
                inflate_ms_ = DeviceReadSet::ms_since(t0);
            }
            cv_.notify_all();
            if (!err.empty() || end) break;
        }
        inflateEnd(&zs);
    }

    const MappedText &t_;
    std::string path_;
    int64_t chunk_;
    palace_ctx *ctx_ = nullptr;
    uint8_t *buf_[kRing] = {nullptr, nullptr, nullptr};
    int64_t len_[kRing] = {0, 0, 0};
    uint64_t head_ = 0, tail_ = 0;
    bool taken_ = false, done_ = false, stop_ = false;
    double inflate_ms_ = 0;
    std::string err_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread th_;
};

// The device path: true = the file's reads are in the set; false = declined (the set is as it was).  A device error, or a parser
// out of room, is thrown.
inline bool ingest_gzip_device(DeviceReadSet &rs, palace_ctx *ctx, const MappedText &t, const std::string &path)
{
    const palace_fastq_cursor before = rs.cursor();
    rs.start_file();
    palace_gzip_params prm{0, 0, 0, 0};
#ifdef PALACE_TEST_HOOKS
    if (const char *v = std::getenv("PALACE_EREF_GZ_STRIDE")) prm.stride = std::atoll(v);    // test builds only
    if (const char *v = std::getenv("PALACE_EREF_GZ_SPAN")) prm.span = std::atoll(v);
#endif
    struct Sink {
        DeviceReadSet *rs;
        std::exception_ptr err;
        static int take(void *user, const uint8_t *d_text, int64_t n, int last)
        {
            Sink *self = static_cast<Sink *>(user);
            try {
                const int64_t W = self->rs->window();
                int64_t p = 0;
                do {                                                         // (windows start 16-byte aligned: W is a multiple of 16)
                    const int64_t w = std::min(W, n - p);
                    self->rs->parse_at(d_text + p, w, last && p + w == n);
                    p += w;
                } while (p < n);
            } catch (...) {
                self->err = std::current_exception();
                return 1;
            }
            return 0;
        }
    } sink{&rs, nullptr};
    palace_gzip_stats st;
    const double parse0 = rs.times.parse;
    rs.ck(palace_gzip_inflate(ctx, reinterpret_cast<const uint8_t *>(t.data), static_cast<int64_t>(t.size), &prm, &Sink::take, &sink, &st),
          "palace_gzip_inflate");
    if (sink.err) std::rethrow_exception(sink.err);
    if (rs.timed()) {
        std::fprintf(stderr, "[eref] gzip on the device: %s: %s; chunks found %lld, accepted %lld, false hits %lld, rounds %lld, members %lld, "
                     "spans %lld, batches %lld, fallback %d; upload %.1f ms, find %.1f ms, size %.1f ms, decode %.1f ms, chain %.1f ms, "
                     "resolve %.1f ms, crc %.1f ms, parse %.1f ms\n", path.c_str(), st.fallback ? "declined, zlib on the host decides" : "device path",
                     static_cast<long long>(st.chunks_found), static_cast<long long>(st.chunks_accepted), static_cast<long long>(st.false_hits),
                     static_cast<long long>(st.rounds), static_cast<long long>(st.members), static_cast<long long>(st.spans),
                     static_cast<long long>(st.batches), st.fallback, st.ms_upload, st.ms_find, st.ms_size, st.ms_decode, st.ms_chain, st.ms_resolve,
                     st.ms_crc, rs.times.parse - parse0);
        rs.times.h2d += st.ms_upload;
        rs.times.inflate += st.ms_find + st.ms_size + st.ms_decode + st.ms_chain + st.ms_resolve;
        rs.times.crc += st.ms_crc;
    }
    if (st.fallback) rs.rewind(before);
    return st.fallback == 0;
}

inline void ingest_gzip(DeviceReadSet &rs, palace_ctx *ctx, const MappedText &t, const std::string &path)
{
    if (ingest_gzip_device(rs, ctx, t, path)) return;
    rs.start_file();
    GzipProducer prod(ctx, t, path, rs.window());
    for (;;) {
        int64_t n = 0;
        bool last = false;
        const uint8_t *src = prod.next(&n, &last);
        const auto t0 = std::chrono::steady_clock::now();
        if (n) rs.ck(palace_h2d(ctx, rs.text(), src, static_cast<size_t>(n)), "text upload");
        rs.times.h2d += DeviceReadSet::ms_since(t0);
        rs.parse(n, last);
        if (last) break;
    }
    rs.times.inflate += prod.inflate_ms();
}

}  // namespace palace_host
