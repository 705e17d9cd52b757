// The host side's device plumbing, stated once for every executable: the throw-on-error call, the owner of a step's device
// allocations, the out-of-room exception, the two sentences of a text input, guards for page-locked buffers and opaque handles, the
// stage clock of traced runs, the upload of a list of names and the line starts of a text.  Nothing here knows a file format; it
// needs include/palace_hip.h, mapped_file.hpp and the standard library.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_hip.h"
#include "mapped_file.hpp"

namespace palace_host {

// a device call that must not fail: `<what>: <the library's message>`
inline void ck(int rc, const char *what)
{
    if (rc) throw std::runtime_error(std::string(what) + ": " + palace_last_error());
}

// ... as the readers of fastq_gz.hpp and depth_read.hpp say it: `device error (<what>): <the library's message>`
inline void ck_device_error(int rc, const char *what)
{
    if (rc) throw std::runtime_error(std::string("device error (") + what + "): " + palace_last_error());
}

// the same for the tools that name the failed call itself (split_fastg, make_fa_from_path)
struct Failure : std::runtime_error { using std::runtime_error::runtime_error; };
#define HIP_OK(call)                                                                                               \
    do {                                                                                                           \
        if ((call) != PALACE_OK) throw palace_host::Failure(std::string(#call " failed: ") + palace_last_error()); \
    } while (0)

// a text input of a tool: `cannot open <path>`, whatever kept it from being mapped
inline void open_text(MappedText &t, const std::string &path)
{
    try { t.open(path); }
    catch (const std::exception &) { throw Failure("cannot open " + path); }
}
// a text outside its grammar: `<file>: line <n>: <reason>`
[[noreturn]] inline void line_fault(const std::string &file, int64_t line, const std::string &reason)
{
    throw Failure(file + ": line " + std::to_string(line) + ": " + reason);
}

// thrown when the device cannot hold what a mode keeps there; the text is the scope's (it names the mode's way out, if there is one)
struct DeviceNoRoom : std::runtime_error { using std::runtime_error::runtime_error; };
using NoRoomText = std::string (*)(size_t bytes, const char *what, const char *err);
inline std::string no_room_plain(size_t, const char *, const char *err) { return std::string("palace_malloc: ") + err; }
inline std::string no_room_device_error(size_t, const char *what, const char *err) { return std::string("device error (") + what + "): " + err; }
inline std::string no_room_does_not_fit(size_t bytes, const char *what, const char *err)
{
    return std::string(what) + " (" + std::to_string(bytes) + " bytes) does not fit the device: " + err;
}

// The device allocations of one step: freed when it leaves -- on the normal path and when unwinding -- unless handed on (keep) or
// given back early.  A request for 0 bytes allocates 1, so every array has an address.
struct DeviceScope {
    palace_ctx *ctx;
    NoRoomText no_room;
    std::vector<void *> owned;
    explicit DeviceScope(palace_ctx *c, NoRoomText text = no_room_plain) : ctx(c), no_room(text) {}
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    ~DeviceScope() { for (void *p : owned) palace_free(ctx, p); }
    void *alloc(size_t bytes, const char *what)
    {
        void *p = nullptr;
        if (palace_malloc(ctx, bytes ? bytes : 1, &p)) throw DeviceNoRoom(no_room(bytes, what, palace_last_error()));
        owned.push_back(p);
        return p;
    }
    template <class T> T *array(size_t n, const char *what) { return static_cast<T *>(alloc(n * sizeof(T), what)); }
    // a new array holding src[0 .. n)
    template <class T> T *upload(const T *src, size_t n, const char *what, const char *copy_what = "palace_h2d")
    {
        T *p = array<T>(n, what);
        if (n) ck(palace_h2d(ctx, p, src, n * sizeof(T)), copy_what);
        return p;
    }
    void give_back(const void *p) { palace_free(ctx, forget(p)); }
    void keep(const void *p) { forget(p); }                                   // (the caller's from here on)
    void keep_all() { owned.clear(); }

private:
    void *forget(const void *p)
    {
        const auto it = std::find(owned.begin(), owned.end(), p);
        void *q = *it;
        owned.erase(it);
        return q;
    }
};

// a page-locked host buffer
struct PinnedBuffer {
    palace_ctx *ctx;
    void *p = nullptr;
    PinnedBuffer(palace_ctx *c, size_t bytes, const char *what = "palace_host_alloc") : ctx(c) { ck(palace_host_alloc(ctx, bytes, &p), what); }
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { if (p) palace_host_free(ctx, p); }
};

// an opaque handle of the library (palace_bam_names, palace_fasta_names, palace_depth_text): `h` is filled by its _create call
template <class H, int (*Destroy)(palace_ctx *, H *)>
struct DeviceHandle {
    palace_ctx *ctx;
    H *h = nullptr;
    explicit DeviceHandle(palace_ctx *c) : ctx(c) {}
    DeviceHandle(const DeviceHandle &) = delete;
    DeviceHandle &operator=(const DeviceHandle &) = delete;
    ~DeviceHandle() { if (h) Destroy(ctx, h); }
};
using BamNamesHandle = DeviceHandle<palace_bam_names, palace_bam_names_destroy>;
using FastaNamesHandle = DeviceHandle<palace_fasta_names, palace_fasta_names_destroy>;
using DepthTextHandle = DeviceHandle<palace_depth_text, palace_depth_text_destroy>;

// The stage clock of a traced run: lap() adds the time since the last lap to *acc, waiting for the device first when asked to.  Off
// (an untraced run), it does nothing: no wait, no time.
struct StageClock {
    using clk = std::chrono::steady_clock;
    palace_ctx *ctx;
    bool on;
    clk::time_point t0 = clk::now();
    void restart() { t0 = clk::now(); }
    void lap(double *acc, bool wait_for_device)
    {
        if (!on) return;
        if (wait_for_device) ck(palace_sync(ctx), "palace_sync");
        const auto t1 = clk::now();
        *acc += std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
    }
};

// names as one blob and n + 1 offsets into it, uploaded into `scope`
struct DeviceNames { uint8_t *blob; int64_t *off; };
inline DeviceNames upload_names(DeviceScope &scope, const std::vector<std::string> &names, const char *what, const char *copy_what)
{
    std::vector<int64_t> off(names.size() + 1, 0);
    std::string blob;
    for (size_t t = 0; t < names.size(); t++) { blob += names[t]; off[t + 1] = static_cast<int64_t>(blob.size()); }
    DeviceNames d;
    d.blob = scope.upload(reinterpret_cast<const uint8_t *>(blob.data()), blob.size(), what, copy_what);
    d.off = scope.upload(off.data(), off.size(), what, copy_what);
    return d;
}

// the lines of the text d_text[0 .. n) (readqc, filter_result): one call of palace_sam_lines counts them, one writes their n_lines + 1
// starts into an array of `scope` (named `what` where it does not fit).  res: the five result words of the second call
struct TextLines { int64_t *d_start; int64_t n_lines; int64_t res[5]; };
inline TextLines text_lines(palace_ctx *ctx, DeviceScope &scope, const uint8_t *d_text, int64_t n, const char *what)
{
    TextLines l{};
    const size_t sb = palace_sam_scratch_bytes(n);
    void *d_scratch = scope.alloc(sb, "the lines' scratch");
    HIP_OK(palace_sam_lines(ctx, d_text, n, d_scratch, sb, nullptr, 0, l.res));
    l.n_lines = l.res[0];
    l.d_start = scope.array<int64_t>(static_cast<size_t>(l.n_lines) + 1, what);
    HIP_OK(palace_sam_lines(ctx, d_text, n, d_scratch, sb, l.d_start, l.n_lines + 1, l.res));
    scope.give_back(d_scratch);
    return l;
}

}  // namespace palace_host
