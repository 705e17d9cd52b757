// An output text that is made on the device goes to its file in windows: window w is computed and copied back while window w - 1 is
// written (make_fa_from_path, make_final_fa, readqc).  Two device windows, two page-locked buffers, the library's marks 0 and 1.
// Nothing here knows what the text is: the tool's `produce` makes the bytes [lo, hi) of it in the device window it is handed.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <string>

#include "device_scope.hpp"

namespace palace_host {

// bytes of output text per window: the variable's value where it is a positive number, else 256 MiB
inline int64_t window_bytes(const char *env_name)
{
    const char *e = std::getenv(env_name);
    const long long v = (e && *e) ? std::atoll(e) : 0;
    return v > 0 ? static_cast<int64_t>(v) : (256ll << 20);
}

// an open file that is closed when the scope is left early -- and removed, where a path is given; release() before the regular fclose
struct FileGuard {
    std::FILE *f;
    const char *remove_path = nullptr;
    ~FileGuard() { if (f) { std::fclose(f); if (remove_path) std::remove(remove_path); } }
    void release() { f = nullptr; }
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
