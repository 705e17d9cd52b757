// An output text that is made on the device goes to its file in windows: window w is computed and copied back while window w - 1 is
// written (WindowWriter: make_fa_from_path, make_final_fa, filter_result, readqc, faidx).  Two device windows, two page-locked
// buffers, the library's marks 0 and 1.  Nothing there knows what the text is: the tool's `produce` makes the bytes [lo, hi) of it in
// the device window it is handed.  Beside it, what those tools and split_fastg share around the text: PendingOutputs, the files that
// get their names only when complete (all six), PathsText, the headers and places of a text of paths (the three FASTA writers), and
// device_to_file, a device buffer to a file in pieces (split_fastg's text, the `.fai` rows).
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>
#include <string_view>
#include <vector>

#include "device_scope.hpp"

namespace palace_host {

// bytes of output text per window: the variable's value where it is a positive number, else 256 MiB
inline int64_t window_bytes(const char *env_name)
{
    const char *e = std::getenv(env_name);
    const long long v = (e && *e) ? std::atoll(e) : 0;
    return v > 0 ? static_cast<int64_t>(v) : (256ll << 20);
}

// The output files of a run.  A file is written as `<path>.tmp` and gets its name only when every file of the run is complete
// (make_final_fa, filter_result, readqc) -- or, in place, under its own name, where the output exists, empty, from the start
// (make_fa_from_path, split_fastg).  Leaving early closes what is open and removes every temporary; a file in place stays as it is.
// The steps say which file failed and throw nothing: the sentence is the tool's.
struct PendingOutputs {
    struct File { std::string path, name; std::FILE *f; };      // name: what is open -- the temporary, or the path itself
    std::vector<File> files;
    PendingOutputs() = default;
    PendingOutputs(const PendingOutputs &) = delete;
    PendingOutputs &operator=(const PendingOutputs &) = delete;
    ~PendingOutputs()
    {
        for (File &o : files) {
            if (o.f) std::fclose(o.f);
            if (o.name != o.path) std::remove(o.name.c_str());  // (renamed already: nothing to remove)
        }
    }
    // the open file (files.back(), whose name is what a message calls it)
    std::FILE *open(const std::string &path, bool in_place = false)
    {
        const std::string name = in_place ? path : path + ".tmp";
        std::FILE *f = std::fopen(name.c_str(), "wb");
        if (!f) throw Failure("cannot write " + name);
        files.push_back(File{path, name, f});
        return f;
    }
    // every file closed; the name of the first that could not be, or nullptr
    const std::string *close()
    {
        const std::string *bad = nullptr;
        for (File &o : files)
            if (o.f) { if (std::fclose(o.f) != 0 && !bad) bad = &o.name; o.f = nullptr; }
        return bad;
    }
    // every temporary to its path; the name of the first that could not be, or nullptr
    const std::string *rename()
    {
        for (File &o : files)
            if (o.name != o.path) { if (std::rename(o.name.c_str(), o.path.c_str()) != 0) return &o.name; o.name = o.path; }
        return nullptr;
    }
    bool commit() { return !close() && !rename(); }
};

// a device buffer of `bytes` bytes to the file, in pieces (split_fastg's text, the `.fai` rows)
inline void device_to_file(palace_ctx *ctx, const uint8_t *d, int64_t bytes, std::FILE *f, const std::string &path)
{
    const int64_t piece = 64ll << 20;
    std::vector<uint8_t> buf(static_cast<size_t>(bytes < piece ? bytes : piece));
    for (int64_t at = 0; at < bytes; at += piece) {
        const size_t k = static_cast<size_t>(bytes - at < piece ? bytes - at : piece);
        HIP_OK(palace_d2h(ctx, buf.data(), d + at, k));
        if (std::fwrite(buf.data(), 1, k, f) != k) throw Failure("cannot write " + path);
    }
}

// The plan of an output text of paths (make_fa_from_path, make_final_fa, filter_result) as palace_path_fasta_write and
// palace_final_fasta_write take it: the headers one behind the other, their offsets, and every path's place in the text -- a written
// path takes its header, its sequence and 3 bytes, a skipped one none.  What the header is and when a path is skipped is the tool's.
struct PathsText {
    std::string hdr;
    std::vector<int64_t> hdr_off{0}, path_out{0};
    void add(std::string_view header, int64_t sequence_length)
    {
        hdr.append(header);
        hdr_off.push_back(static_cast<int64_t>(hdr.size()));
        path_out.push_back(path_out.back() + static_cast<int64_t>(header.size()) + sequence_length + 3);
    }
    void skip() { hdr_off.push_back(hdr_off.back()); path_out.push_back(path_out.back()); }
    struct OnDevice { const uint8_t *d_hdr; const int64_t *d_hdr_off, *d_path_out; int64_t total; };
    OnDevice upload(DeviceScope &scope) const
    {
        OnDevice d;
        d.total = path_out.back();
        d.d_hdr = scope.upload(reinterpret_cast<const uint8_t *>(hdr.data()), hdr.size(), "the headers");
        d.d_hdr_off = scope.upload(hdr_off.data(), hdr_off.size(), "the headers' offsets");
        d.d_path_out = scope.upload(path_out.data(), path_out.size(), "the paths' places");
        return d;
    }
};

struct WindowWriter {
    palace_ctx *ctx;
    int64_t win;                             // a window's bytes: what the variable says, but no more than the longest text (and not 0)
    uint8_t *d_win[2];                       // (the caller's scope owns them)
    PinnedBuffer pin0, pin1;
    WindowWriter(palace_ctx *c, DeviceScope &dev, const char *env_name, int64_t longest_total)
        : ctx(c), win(std::min(window_bytes(env_name), std::max<int64_t>(longest_total, 1))),
          d_win{dev.array<uint8_t>(static_cast<size_t>(win), "an output window"), dev.array<uint8_t>(static_cast<size_t>(win), "an output window")},
          pin0(c, static_cast<size_t>(win), "no pinned memory for an output window"), pin1(c, static_cast<size_t>(win), "no pinned memory for an output window")
    {
    }

    // the text's `total` bytes to f; produce(lo, hi, d_window) enqueues the making of bytes [lo, hi).  One text after the other may be
    // written from the same buffers: every window of a text has reached its file when this returns.
    template <class Produce>
    void write(int64_t total, std::FILE *f, const std::string &name, Produce produce)
    {
        void *const pin[2] = {pin0.p, pin1.p};
        auto flush = [&](int64_t w) {
            const int64_t lo = w * win, hi = lo + win < total ? lo + win : total;
            HIP_OK(palace_mark_wait(ctx, static_cast<int>(w & 1)));
            if (std::fwrite(pin[w & 1], 1, static_cast<size_t>(hi - lo), f) != static_cast<size_t>(hi - lo)) throw Failure("cannot write " + name);
        };
        const int64_t n_win = (total + win - 1) / win;
        for (int64_t w = 0; w < n_win; w++) {
            const int64_t lo = w * win, hi = lo + win < total ? lo + win : total;
            produce(lo, hi, d_win[w & 1]);
            HIP_OK(palace_d2h_async(ctx, pin[w & 1], d_win[w & 1], static_cast<size_t>(hi - lo)));
            HIP_OK(palace_mark(ctx, static_cast<int>(w & 1)));
            if (w) flush(w - 1);
        }
        if (n_win) flush(n_win - 1);
    }
};

}  // namespace palace_host
