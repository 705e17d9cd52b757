// device_scope.hpp, mapped_file.hpp, output_windows.hpp, the duplicate helper of fasta_device.hpp, the member writer's arithmetic and the BGZF
// batch reader (bgzf_read_device.hpp: its "device" inflates with zlib and can be told to refuse members) on their own
// (tests/test_host_device_scope.py; also built with the host sanitizers).  No device and no libpalace_hip.so: the few palace_* calls
// the headers make are stubs here that count their calls, remember what is live, queue the asynchronous copies and can be told to
// fail.  `device_scope_selftest <scratch directory>` prints one line per failed check and `ok <checks>` at the end; exit code 1 if
// any check failed.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <sys/stat.h>
#include <string>
#include <vector>

#include "bai.hpp"
#include "bam_stream_device.hpp"
#include "bgzf_members_device.hpp"
#include "bgzf_read_device.hpp"
#include "device_scope.hpp"
#include "fasta_device.hpp"
#include "mapped_file.hpp"
#include "output_windows.hpp"
#include "sam_device.hpp"

using namespace palace_host;

namespace {

struct Stub {
    int mallocs = 0, frees = 0, host_allocs = 0, host_frees = 0, copies = 0, copies_back = 0, syncs = 0, destroys = 0, bad_frees = 0;
    int fail_malloc = 0;                            // the k-th palace_malloc from now fails (0: none)
    bool fail_sync = false, fail_host_alloc = false;
    std::map<void *, size_t> live, live_host;      // pointer -> bytes asked for
    std::vector<size_t> asked;
    struct Copy { void *dst; const void *src; size_t bytes; };
    std::vector<Copy> queue;                        // palace_d2h_async calls in order; the first queue_done of them have happened
    size_t queue_done = 0, mark_at[2] = {0, 0};     // mark k stands behind the first mark_at[k] copies
    bool in_flight[2] = {false, false};             // mark k was set and not yet waited for
    std::vector<size_t> refuse;                     // palace_bgzf_inflate refuses these members, counted over its calls since reset()
    size_t members_seen = 0;
    void reset() { *this = Stub(); }
} stub;
const char *kErr = "out of memory (stub)";

int checks = 0, failed = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        checks++;                                                                 \
        if (!(cond)) { failed++; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

}  // namespace

extern "C" {
const char *palace_last_error(void) { return kErr; }
int palace_malloc(palace_ctx *, size_t bytes, void **d_out)
{
    stub.mallocs++;
    stub.asked.push_back(bytes);
    if (stub.fail_malloc && --stub.fail_malloc == 0) return -1;
    *d_out = std::malloc(bytes);
    stub.live[*d_out] = bytes;
    return 0;
}
int palace_free(palace_ctx *, void *p)
{
    stub.frees++;
    if (!stub.live.erase(p)) { stub.bad_frees++; return -1; }
    std::free(p);
    return 0;
}
int palace_host_alloc(palace_ctx *, size_t bytes, void **h_out)
{
    stub.host_allocs++;
    if (stub.fail_host_alloc) return -1;
    *h_out = std::malloc(bytes ? bytes : 1);
    stub.live_host[*h_out] = bytes;
    return 0;
}
int palace_host_free(palace_ctx *, void *p)
{
    stub.host_frees++;
    if (!stub.live_host.erase(p)) { stub.bad_frees++; return -1; }
    std::free(p);
    return 0;
}
int palace_h2d(palace_ctx *, void *d_dst, const void *h_src, size_t bytes)
{
    stub.copies++;
    std::memcpy(d_dst, h_src, bytes);
    return 0;
}
int palace_d2h(palace_ctx *, void *h_dst, const void *d_src, size_t bytes)
{
    stub.copies_back++;
    std::memcpy(h_dst, d_src, bytes);
    return 0;
}
int palace_sync(palace_ctx *) { stub.syncs++; return stub.fail_sync ? -1 : 0; }
// the stream of the stubs: a copy back is only queued; it happens when a mark behind it is waited for
int palace_d2h_async(palace_ctx *, void *h_dst, const void *d_src, size_t bytes)
{
    stub.queue.push_back(Stub::Copy{h_dst, d_src, bytes});
    return 0;
}
int palace_mark(palace_ctx *, int idx)
{
    stub.mark_at[idx & 1] = stub.queue.size();
    stub.in_flight[idx & 1] = true;
    return 0;
}
int palace_mark_wait(palace_ctx *, int idx)
{
    for (; stub.queue_done < stub.mark_at[idx & 1]; stub.queue_done++) {
        const Stub::Copy &c = stub.queue[stub.queue_done];
        std::memcpy(c.dst, c.src, c.bytes);
    }
    stub.in_flight[idx & 1] = false;
    return 0;
}
// the "device" decoder: raw zlib inflate of every member, status 0; a refused member gets status 1 and its bytes are not touched
int palace_bgzf_inflate(palace_ctx *, const uint8_t *d_in, int64_t n_members, const int64_t *d_in_off, const int32_t *d_in_len, const int64_t *d_out_off,
                        const int32_t *d_out_len, uint8_t *d_out, int32_t *d_status)
{
    for (int64_t j = 0; j < n_members; j++, stub.members_seen++) {
        d_status[j] = 1;
        if (std::count(stub.refuse.begin(), stub.refuse.end(), stub.members_seen)) continue;
        d_status[j] = 0;
        if (d_out_len[j] == 0) continue;
        z_stream zs{};
        if (inflateInit2(&zs, -15) != Z_OK) return -1;
        zs.next_in = const_cast<Bytef *>(d_in + d_in_off[j]); zs.avail_in = static_cast<uInt>(d_in_len[j]);
        zs.next_out = d_out + d_out_off[j]; zs.avail_out = static_cast<uInt>(d_out_len[j]);
        if (inflate(&zs, Z_FINISH) != Z_STREAM_END || zs.avail_out != 0) d_status[j] = 1;
        inflateEnd(&zs);
    }
    return 0;
}
int palace_crc32_members(palace_ctx *, const uint8_t *d_data, int64_t n_members, const int64_t *d_off, const int32_t *d_len, uint32_t *d_crc)
{
    for (int64_t j = 0; j < n_members; j++)
        d_crc[j] = static_cast<uint32_t>(::crc32(::crc32(0L, Z_NULL, 0), d_data + d_off[j], static_cast<uInt>(d_len[j])));
    return 0;
}
int palace_bam_names_destroy(palace_ctx *, palace_bam_names *) { stub.destroys++; return 0; }
int palace_fasta_names_destroy(palace_ctx *, palace_fasta_names *) { stub.destroys++; return 0; }
int palace_depth_text_destroy(palace_ctx *, palace_depth_text *) { stub.destroys++; return 0; }
}

namespace {

palace_ctx *const ctx = nullptr;                    // (the stubs never look at it)

// the out-of-room texts the executables print, written out in full: --bam-gpu, bamsort, the SAM front end, split_fastg / make_fa_from_path,
// the depth file writer, and the readers of depth_read.hpp / fastq_gz.hpp
struct Style { const char *name; NoRoomText text; std::string (*want)(const std::string &bytes, const std::string &what); };
const Style kStyles[] = {
    {"bam-gpu", bam_gpu_no_room, [](const std::string &b, const std::string &w) {
         return "--bam-gpu keeps the whole inflated BAM on the device and cannot allocate " + b + " bytes for " + w +
                " (out of memory (stub)); run without --bam-gpu to load the BAM on the host";
     }},
    {"bamsort", bamsort_no_room, [](const std::string &b, const std::string &w) {
         return "the inflated BAM, the sorted stream, the per-record arrays and one batch of members are kept on the device, and " + b + " bytes for " + w +
                " cannot be allocated (out of memory (stub)); there is no host path, a BAM larger than device memory is out of scope";
     }},
    {"sam", sam_no_room, [](const std::string &b, const std::string &w) {
         return "the SAM text, the BAM stream, 24 bytes per line and 8 per record are kept on the device, and " + b + " bytes for " + w +
                " cannot be allocated (out of memory (stub)); there is no host path, a text larger than device memory is out of scope";
     }},
    {"does-not-fit", no_room_does_not_fit, [](const std::string &b, const std::string &w) { return w + " (" + b + " bytes) does not fit the device: out of memory (stub)"; }},
    {"plain", no_room_plain, [](const std::string &, const std::string &) { return std::string("palace_malloc: out of memory (stub)"); }},
    {"device-error", no_room_device_error, [](const std::string &, const std::string &w) { return "device error (" + w + "): out of memory (stub)"; }},
};

int failing_call() { return -1; }

void test_scope()
{
    const int N = 6;
    {   // leaves normally: every pointer freed exactly once
        stub.reset();
        {
            DeviceScope dev(ctx);
            for (int i = 1; i <= N; i++) dev.alloc(static_cast<size_t>(100 * i), "the thing");
            CHECK(stub.mallocs == N && stub.frees == 0 && stub.live.size() == static_cast<size_t>(N));
        }
        CHECK(stub.frees == N && stub.live.empty() && stub.bad_frees == 0);
    }
    for (const Style &s : kStyles)
        for (int k = 1; k <= N; k++) {   // the k-th allocation fails: the k - 1 before it are freed exactly once, the text is the style's
            stub.reset();
            stub.fail_malloc = k;
            bool no_room = false;
            std::string text;
            try {
                DeviceScope dev(ctx, s.text);
                for (int i = 1; i <= N; i++) dev.alloc(static_cast<size_t>(100 * i), "the thing");
            } catch (const DeviceNoRoom &e) { no_room = true; text = e.what(); }
            CHECK(no_room);
            CHECK(text == s.want(std::to_string(100 * k), "the thing"));
            CHECK(stub.mallocs == k && stub.frees == k - 1 && stub.live.empty() && stub.bad_frees == 0);
        }
    {   // give_back, keep, keep_all, zero bytes, array, upload
        stub.reset();
        void *kept = nullptr, *kept2[2] = {nullptr, nullptr};
        {
            DeviceScope dev(ctx);
            void *a = dev.alloc(10, "a");
            kept = dev.alloc(20, "b");
            void *z = dev.alloc(0, "nothing");
            CHECK(stub.asked.back() == 1 && z != nullptr);
            int32_t *arr = dev.array<int32_t>(7, "seven");
            CHECK(stub.asked.back() == 28 && arr != nullptr);
            const int64_t src[3] = {5, -6, 7};
            const int64_t *up = dev.upload(src, 3, "three");
            CHECK(stub.asked.back() == 24 && stub.copies == 1 && std::memcmp(up, src, 24) == 0);
            dev.upload(src, 0, "none");
            CHECK(stub.asked.back() == 1 && stub.copies == 1);
            dev.give_back(a);
            CHECK(stub.frees == 1 && !stub.live.count(a));
            dev.keep(kept);
            CHECK(stub.frees == 1 && stub.live.count(kept));
        }
        CHECK(stub.mallocs == 6 && stub.frees == 5 && stub.live.size() == 1 && stub.live.count(kept) && stub.bad_frees == 0);
        {
            DeviceScope dev(ctx);
            kept2[0] = dev.alloc(1, "x");
            kept2[1] = dev.alloc(2, "y");
            dev.keep_all();
        }
        CHECK(stub.frees == 5 && stub.live.size() == 3);
        for (void *p : {kept, kept2[0], kept2[1]}) palace_free(ctx, p);
        CHECK(stub.live.empty() && stub.bad_frees == 0);
    }
    {   // names: one blob, n + 1 offsets
        stub.reset();
        {
            DeviceScope dev(ctx);
            const DeviceNames d = upload_names(dev, {"a", "", "chr2"}, "the names", "names");
            const int64_t want[4] = {0, 1, 1, 5};
            CHECK(std::memcmp(d.blob, "achr2", 5) == 0 && std::memcmp(d.off, want, 32) == 0 && stub.asked == (std::vector<size_t>{5, 32}));
            const DeviceNames e = upload_names(dev, {}, "the names", "names");
            CHECK(e.off[0] == 0 && e.blob != nullptr && stub.asked == (std::vector<size_t>{5, 32, 1, 8}));
        }
        CHECK(stub.live.empty() && stub.frees == 4 && stub.bad_frees == 0);
    }
    {   // ck: today's text
        std::string text;
        try { ck(-1, "palace_whatever"); } catch (const std::runtime_error &e) { text = e.what(); }
        CHECK(text == "palace_whatever: out of memory (stub)");
        ck(0, "fine");
        text.clear();
        try { HIP_OK(failing_call()); } catch (const Failure &e) { text = e.what(); }
        CHECK(text == "failing_call() failed: out of memory (stub)");
    }
}

void test_guards()
{
    stub.reset();
    {
        PinnedBuffer pin(ctx, 4096);
        CHECK(pin.p != nullptr && stub.host_allocs == 1 && stub.host_frees == 0 && stub.live_host.size() == 1);
    }
    CHECK(stub.host_frees == 1 && stub.live_host.empty() && stub.bad_frees == 0);
    stub.fail_host_alloc = true;
    std::string text;
    try { PinnedBuffer pin(ctx, 4096, "no pinned memory for an output window"); } catch (const std::runtime_error &e) { text = e.what(); }
    CHECK(text == "no pinned memory for an output window: out of memory (stub)" && stub.host_frees == 1);

    stub.reset();
    int thing = 0;
    { BamNamesHandle h(ctx); }
    { FastaNamesHandle h(ctx); }
    { DepthTextHandle h(ctx); }
    CHECK(stub.destroys == 0);                      // a handle that was never made is not destroyed
    { BamNamesHandle h(ctx); h.h = reinterpret_cast<palace_bam_names *>(&thing); }
    CHECK(stub.destroys == 1);
    { FastaNamesHandle h(ctx); h.h = reinterpret_cast<palace_fasta_names *>(&thing); }
    CHECK(stub.destroys == 2);
    { DepthTextHandle h(ctx); h.h = reinterpret_cast<palace_depth_text *>(&thing); }
    CHECK(stub.destroys == 3);
}

void test_clock()
{
    stub.reset();
    double acc = 0;
    StageClock off{ctx, false};
    off.restart();
    off.lap(&acc, true);
    off.lap(&acc, false);
    CHECK(stub.syncs == 0 && acc == 0);
    StageClock on{ctx, true};
    on.restart();
    for (int i = 0; i < 3; i++) on.lap(&acc, true);
    CHECK(stub.syncs == 3 && acc >= 0);
    on.lap(&acc, false);
    CHECK(stub.syncs == 3);
    stub.fail_sync = true;
    std::string text;
    try { on.lap(&acc, true); } catch (const std::runtime_error &e) { text = e.what(); }
    CHECK(text == "palace_sync: out of memory (stub)");
    stub.syncs = 0;
    off.lap(&acc, true);                            // (off: not even asked)
    CHECK(stub.syncs == 0);
}

void test_mapped_file(const std::string &dir)
{
    const std::string missing = dir + "/missing", empty = dir + "/empty", big = dir + "/big";
    for (int bam = 0; bam < 2; bam++) {
        std::string text;
        try {
            if (bam) { MappedFile f(missing, MapHint::sequential, "Failed to open BAM ", "Failed to read BAM "); }
            else { MappedText f(missing); }
        } catch (const std::runtime_error &e) { text = e.what(); }
        CHECK(text == (bam ? "Failed to open BAM " : "cannot open ") + missing);
    }
    { std::ofstream f(empty, std::ios::binary); }
    for (MapHint hint : {MapHint::none, MapHint::populate, MapHint::sequential}) {
        MappedFile f(empty, hint);
        CHECK(f.size == 0 && f.data == nullptr && f.bytes() == nullptr);
    }
    std::string content(70000, '\0');
    for (size_t i = 0; i < content.size(); i++) content[i] = static_cast<char>((i * 2654435761u) >> 13);
    { std::ofstream f(big, std::ios::binary); f.write(content.data(), static_cast<std::streamsize>(content.size())); }
    for (MapHint hint : {MapHint::none, MapHint::populate, MapHint::sequential}) {
        MappedFile f;
        f.open(big, hint);
        CHECK(f.size == content.size() && std::memcmp(f.data, content.data(), content.size()) == 0);
    }
}

std::string file_bytes(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

// output_windows.hpp: one writer, 64-byte windows, texts of several lengths one after the other from the same buffers
void test_windows(const std::string &dir)
{
    const char *unset = "PALACE_SELFTEST_WINDOW_UNSET", *var = "PALACE_SELFTEST_WINDOW";
    unsetenv(unset);
    CHECK(window_bytes(unset) == (256ll << 20));
    for (const char *v : {"", "0", "-5", "abc"}) {
        setenv(var, v, 1);
        CHECK(window_bytes(var) == (256ll << 20));
    }
    setenv(var, "64", 1);
    CHECK(window_bytes(var) == 64);

    const int64_t win = 64;
    stub.reset();
    {
        DeviceScope dev(ctx);
        {   // the window is no longer than the longest text and never empty
            WindowWriter none(ctx, dev, unset, 0), small(ctx, dev, var, 10), whole(ctx, dev, unset, 1000);
            CHECK(none.win == 1 && small.win == 10 && whole.win == 1000);
            CHECK(stub.asked == (std::vector<size_t>{1, 1, 10, 10, 1000, 1000}) && stub.live_host.size() == 6);
        }
        CHECK(stub.live_host.empty() && stub.host_allocs == 6 && stub.host_frees == 6);
        WindowWriter ww(ctx, dev, var, 3 * win);
        CHECK(ww.win == win && stub.mallocs == 8 && stub.host_allocs == 8 && stub.live_host.size() == 2);
        for (const auto &kv : stub.live_host) CHECK(kv.second == static_cast<size_t>(win));
        std::vector<char> text(static_cast<size_t>(3 * win));
        for (size_t i = 0; i < text.size(); i++) text[i] = static_cast<char>((i * 2654435761u) >> 11);
        for (int64_t total : {int64_t{0}, int64_t{1}, win, win + 1, 3 * win}) {
            const std::string path = dir + "/windows_" + std::to_string(total);
            std::FILE *f = std::fopen(path.c_str(), "wb");
            CHECK(f != nullptr);
            const size_t copies = stub.queue.size();
            int64_t next = 0;
            ww.write(total, f, path, [&](int64_t lo, int64_t hi, uint8_t *d_win) {
                CHECK(lo == next && hi == (lo + win < total ? lo + win : total) && hi > lo);
                const int k = d_win == ww.d_win[1] ? 1 : 0;
                CHECK(d_win == ww.d_win[k] && k == ((lo / win) & 1));
                CHECK(!stub.in_flight[k]);                                   // what was copied out of this window before has arrived
                std::memset(d_win, 0xee, static_cast<size_t>(win));
                std::memcpy(d_win, text.data() + lo, static_cast<size_t>(hi - lo));
                next = hi;
            });
            CHECK(next == total && stub.queue.size() - copies == static_cast<size_t>((total + win - 1) / win));
            CHECK(stub.queue_done == stub.queue.size() && !stub.in_flight[0] && !stub.in_flight[1]);     // nothing is left on its way
            CHECK(std::fclose(f) == 0);
            CHECK(file_bytes(path) == std::string(text.data(), static_cast<size_t>(total)));
        }
        // a file that takes no byte: the stated text, for the first window and for a later one; nothing of it when there is no byte
        std::vector<std::string> targets{dir + "/windows_0"};                // (opened for reading: a write to it fails)
        if (std::FILE *full = std::fopen("/dev/full", "wb")) { std::fclose(full); targets.push_back("/dev/full"); }
        for (const std::string &target : targets)
            for (int64_t total : {int64_t{0}, int64_t{1}, 3 * win}) {
                std::FILE *f = std::fopen(target.c_str(), target == "/dev/full" ? "wb" : "rb");
                CHECK(f != nullptr);
                std::setvbuf(f, nullptr, _IONBF, 0);
                std::string said;
                try {
                    ww.write(total, f, "the name", [&](int64_t lo, int64_t hi, uint8_t *d_win) { std::memcpy(d_win, text.data() + lo, static_cast<size_t>(hi - lo)); });
                } catch (const Failure &e) { said = e.what(); }
                CHECK(said == (total ? "cannot write the name" : ""));
                std::fclose(f);
            }
        CHECK(stub.mallocs == 8 && stub.host_allocs == 8);                   // (the buffers of the start served every text)
    }
    CHECK(stub.live.empty() && stub.live_host.empty() && stub.frees == 8 && stub.host_frees == 8 && stub.bad_frees == 0);
    stub.reset();
    stub.fail_host_alloc = true;                                             // no pinned memory: the label, and the device windows go with the scope
    std::string said;
    try {
        DeviceScope dev(ctx);
        WindowWriter ww(ctx, dev, var, 100);
    } catch (const std::runtime_error &e) { said = e.what(); }
    CHECK(said == "no pinned memory for an output window: out of memory (stub)" && stub.mallocs == 2 && stub.live.empty() && stub.bad_frees == 0);
    stub.reset();
    stub.fail_malloc = 2;
    said.clear();
    try {
        DeviceScope dev(ctx, no_room_does_not_fit);
        WindowWriter ww(ctx, dev, var, 100);
    } catch (const DeviceNoRoom &e) { said = e.what(); }
    CHECK(said == "an output window (64 bytes) does not fit the device: out of memory (stub)" && stub.live.empty() && stub.host_allocs == 0);
}

bool exists(const std::string &path)
{
    struct stat st;
    return ::stat(path.c_str(), &st) == 0;
}

// output_windows.hpp: the headers and places of a text of paths, against sums written out by hand
void test_paths_text()
{
    using V = std::vector<int64_t>;
    stub.reset();
    DeviceScope dev(ctx);
    {   // no path at all
        const PathsText none;
        const PathsText::OnDevice d = none.upload(dev);
        CHECK(d.total == 0 && none.hdr.empty() && none.hdr_off == V{0} && none.path_out == V{0});
        CHECK(d.d_hdr != nullptr && d.d_hdr_off[0] == 0 && d.d_path_out[0] == 0);
        CHECK(stub.asked == (std::vector<size_t>{0 + 1, 8, 8}));             // (0 bytes of headers: an array of 1)
    }
    {   // a skipped path first, between two written ones and last; a header of 0 bytes
        PathsText t;
        t.skip();
        t.add("ab", 10);                                                     // 2 + 10 + 3 = 15
        t.skip();
        t.add("", 4);                                                        // 0 +  4 + 3 =  7
        t.add("xyz", 0);                                                     // 3 +  0 + 3 =  6
        t.skip();
        CHECK(t.hdr == "abxyz");
        CHECK(t.hdr_off == (V{0, 0, 2, 2, 2, 5, 5}));
        CHECK(t.path_out == (V{0, 0, 15, 15, 22, 28, 28}));
        const size_t before = stub.asked.size();
        const PathsText::OnDevice d = t.upload(dev);
        CHECK(d.total == 28 && std::memcmp(d.d_hdr, "abxyz", 5) == 0);
        CHECK(std::memcmp(d.d_hdr_off, t.hdr_off.data(), 7 * 8) == 0 && std::memcmp(d.d_path_out, t.path_out.data(), 7 * 8) == 0);
        CHECK(stub.asked.size() == before + 3 && stub.asked[before] == 5 && stub.asked[before + 1] == 56 && stub.asked[before + 2] == 56);
    }
    {   // only skipped paths: no byte
        PathsText t;
        t.skip();
        t.skip();
        CHECK(t.upload(dev).total == 0 && t.hdr_off == (V{0, 0, 0}) && t.path_out == (V{0, 0, 0}));
    }
    stub.fail_malloc = 2;                                                    // the names of what does not fit
    std::string said;
    try { DeviceScope small(ctx, no_room_does_not_fit); PathsText t; t.add("h", 1); t.upload(small); } catch (const DeviceNoRoom &e) { said = e.what(); }
    CHECK(said == "the headers' offsets (16 bytes) does not fit the device: out of memory (stub)");
}

// output_windows.hpp: files that get their names only when all are complete
void test_pending_outputs(const std::string &dir)
{
    const std::string a = dir + "/pending_a", b = dir + "/pending_b", blocked = dir + "/pending_dir";
    {   // one file
        PendingOutputs o;
        std::FILE *f = o.open(a);
        CHECK(f != nullptr && o.files.back().name == a + ".tmp" && o.files.back().path == a);
        CHECK(std::fputs("one", f) >= 0 && exists(a + ".tmp") && !exists(a));
        CHECK(o.commit());
        CHECK(o.files.back().f == nullptr && o.files.back().name == a);
    }
    CHECK(file_bytes(a) == "one" && !exists(a + ".tmp"));                    // (and the destructor removed nothing)
    {   // two files: closed, something else written, renamed (the order of readqc's reports)
        PendingOutputs o;
        std::fputs("first", o.open(a));
        std::fputs("second", o.open(b));
        CHECK(o.close() == nullptr && file_bytes(a) == "one" && file_bytes(a + ".tmp") == "first" && !exists(b));
        CHECK(o.close() == nullptr);                                         // (nothing is closed twice)
        CHECK(o.rename() == nullptr);
    }
    CHECK(file_bytes(a) == "first" && file_bytes(b) == "second" && !exists(a + ".tmp") && !exists(b + ".tmp"));
    std::remove(a.c_str());
    std::remove(b.c_str());
    {   // left before the commit: every temporary goes, no file gets its name
        PendingOutputs o;
        std::fputs("x", o.open(a));
        std::fputs("y", o.open(b));
        CHECK(exists(a + ".tmp") && exists(b + ".tmp"));
    }
    CHECK(!exists(a) && !exists(b) && !exists(a + ".tmp") && !exists(b + ".tmp"));
    {   // a temporary that cannot be opened: the sentence names it, the one before it goes
        std::string said;
        try {
            PendingOutputs o;
            o.open(a);
            o.open(dir + "/no_such_directory/out");
        } catch (const Failure &e) { said = e.what(); }
        CHECK(said == "cannot write " + dir + "/no_such_directory/out.tmp" && !exists(a + ".tmp"));
    }
    CHECK(::mkdir(blocked.c_str(), 0700) == 0);
    {   // the second rename fails (its target is a directory): failure is reported with the temporary's name, both temporaries are gone
        PendingOutputs o;
        std::fputs("x", o.open(a));
        std::fputs("y", o.open(blocked));
        CHECK(o.close() == nullptr);
        const std::string *bad = o.rename();
        CHECK(bad != nullptr && *bad == blocked + ".tmp");
    }
    CHECK(!exists(a + ".tmp") && !exists(blocked + ".tmp") && file_bytes(a) == "x");           // (the first had its name already)
    std::remove(a.c_str());
    {
        PendingOutputs o;
        std::fputs("x", o.open(a));
        std::fputs("y", o.open(blocked));
        CHECK(!o.commit());
    }
    CHECK(!exists(a + ".tmp") && !exists(blocked + ".tmp"));
    std::remove(a.c_str());
    {   // in place: the file exists, empty, from the start, and stays when the run is left early
        PendingOutputs o;
        o.open(a, true);
        CHECK(o.files.back().name == a && exists(a) && !exists(a + ".tmp"));
    }
    CHECK(exists(a) && file_bytes(a).empty());
    {   // ... and a commit closes it and renames nothing
        PendingOutputs o;
        std::fputs("whole", o.open(a, true));
        CHECK(o.commit() && o.files.back().f == nullptr);
    }
    CHECK(file_bytes(a) == "whole");
    if (std::FILE *full = std::fopen("/dev/full", "wb")) {                   // a file that takes no byte: close names it
        std::fclose(full);
        PendingOutputs o;
        std::fputs("x", o.open(a));
        std::fputs("lost", o.open("/dev/full", true));
        const std::string *bad = o.close();
        CHECK(bad != nullptr && *bad == "/dev/full" && o.files[0].f == nullptr && o.files[1].f == nullptr);       // (both are closed all the same)
    }
    CHECK(!exists(a + ".tmp"));
}

// fasta_device.hpp: the records come to the host once, and only when a flag is set
void test_duplicates()
{
    std::vector<palace_fasta_rec> recs(5);
    for (size_t k = 0; k < recs.size(); k++) recs[k] = palace_fasta_rec{static_cast<int64_t>(10 * k), static_cast<int64_t>(k + 1), 0, 0, 0, 0};
    const char *text = "the text";
    struct Seen { size_t k; int64_t name_off, name_len; const char *text; };
    std::vector<Seen> seen;
    auto note = [&](size_t k, const palace_fasta_rec &r, const char *t) { seen.push_back(Seen{k, r.name_off, r.name_len, t}); };
    stub.reset();
    for_each_duplicate(ctx, std::vector<uint8_t>{}, recs.data(), text, note);
    for_each_duplicate(ctx, std::vector<uint8_t>{0, 0, 0, 0, 0}, recs.data(), text, note);
    CHECK(seen.empty() && stub.copies_back == 0);
    for_each_duplicate(ctx, std::vector<uint8_t>{1, 0, 0, 0, 1}, recs.data(), text, note);
    CHECK(stub.copies_back == 1 && seen.size() == 2);
    CHECK(seen.size() == 2 && seen[0].k == 0 && seen[0].name_off == 0 && seen[0].name_len == 1 && seen[0].text == text);
    CHECK(seen.size() == 2 && seen[1].k == 4 && seen[1].name_off == 40 && seen[1].name_len == 5 && seen[1].text == text);
    seen.clear();
    for_each_duplicate(ctx, std::vector<uint8_t>{0, 0, 1, 0, 0}, recs.data(), text, note);
    CHECK(stub.copies_back == 2 && seen.size() == 1 && seen[0].k == 2 && seen[0].name_off == 20);
    bool stopped = false;                                                    // a tool that faults at the first one sees no second
    seen.clear();
    try {
        for_each_duplicate(ctx, std::vector<uint8_t>{0, 1, 1, 0, 0}, recs.data(), text, [&](size_t k, const palace_fasta_rec &r, const char *t) {
            note(k, r, t);
            line_fault("a.fasta", line_of("x\ny\nz", 4), "twice");
        });
    } catch (const Failure &e) { stopped = std::string(e.what()) == "a.fasta: line 3: twice"; }
    CHECK(stopped && seen.size() == 1 && seen[0].k == 1);
    CHECK(line_of("x\ny\nz", 0) == 1 && line_of("x\ny\nz", 1) == 1 && line_of("x\ny\nz", 2) == 2);
}

// device_scope.hpp: the two sentences of a text input
void test_text_input(const std::string &dir)
{
    std::string said;
    MappedText t;
    try { open_text(t, dir + "/missing"); } catch (const Failure &e) { said = e.what(); }
    CHECK(said == "cannot open " + dir + "/missing");
    open_text(t, dir + "/big");                                              // (test_mapped_file wrote it)
    CHECK(t.size == 70000);
    said.clear();
    try { line_fault("f.txt", 12, "no good"); } catch (const Failure &e) { said = e.what(); }
    CHECK(said == "f.txt: line 12: no good");
}

void test_member_arithmetic()
{
    const uint64_t T = 0xff00;
    for (uint64_t size : {uint64_t{0}, uint64_t{1}, T - 1, T, T + 1, 2 * T})
        for (size_t cap : {size_t{1}, size_t{3}, size_t{8192}}) {
            const size_t n = bgzf_member_count(size), batch = bgzf_batch_members(n, cap);
            CHECK(n == (size + T - 1) / T);
            CHECK(batch >= 1 && batch <= cap && (n == 0 || batch <= n));
            std::vector<int32_t> lens(batch);
            uint64_t sum = 0, at = 0;
            size_t members = 0;
            for (size_t m0 = 0; m0 < n; m0 += batch) {
                const MemberBatch b = bgzf_batch(size, n, batch, m0, lens.data());
                CHECK(b.nm == (n - m0 < batch ? n - m0 : batch));
                CHECK(b.t_beg == at && b.t_beg == m0 * T);
                CHECK(b.t_end == (size < (m0 + b.nm) * T ? size : (m0 + b.nm) * T));
                for (size_t k = 0; k < b.nm; k++) {
                    const bool last = m0 + k + 1 == n;
                    CHECK(lens[k] > 0 && static_cast<uint64_t>(lens[k]) <= T);
                    CHECK(last ? static_cast<uint64_t>(lens[k]) == size - (n - 1) * T : static_cast<uint64_t>(lens[k]) == T);
                    sum += static_cast<uint64_t>(lens[k]);
                }
                at = b.t_end;
                members += b.nm;
            }
            CHECK(members == n && sum == size && at == size);
        }
}

void test_stored_member()
{
    for (uint32_t len : {0u, 1u, 0xff00u}) {
        std::vector<uint8_t> data(len);
        for (uint32_t i = 0; i < len; i++) data[i] = static_cast<uint8_t>((i * 40503u) >> 7);
        const uint32_t crc = static_cast<uint32_t>(::crc32(::crc32(0L, Z_NULL, 0), data.data(), len));
        std::vector<uint8_t> m{0xaa};                // (appended: what is there stays)
        append_stored_member(m, data.data(), len, crc);
        CHECK(m[0] == 0xaa && m.size() == 1 + 18 + 5 + len + 8);
        const size_t total = m.size() - 1;
        CHECK((m[17] | (m[18] << 8)) == static_cast<int>(total - 1));            // BSIZE
        uint32_t got_crc, got_len;
        std::memcpy(&got_crc, m.data() + m.size() - 8, 4);
        std::memcpy(&got_len, m.data() + m.size() - 4, 4);
        CHECK(got_crc == crc && got_len == len);
        z_stream zs{};
        CHECK(inflateInit2(&zs, 15 + 16) == Z_OK);                               // a gzip member: zlib checks CRC-32 and ISIZE itself
        std::vector<uint8_t> out(len + 1);
        zs.next_in = m.data() + 1; zs.avail_in = static_cast<uInt>(total);
        zs.next_out = out.data(); zs.avail_out = static_cast<uInt>(out.size());
        CHECK(inflate(&zs, Z_FINISH) == Z_STREAM_END);
        CHECK(zs.total_out == len && zs.avail_in == 0 && std::equal(data.begin(), data.end(), out.begin()));
        inflateEnd(&zs);
    }
}

// ---- bgzf_read_device.hpp: the batch plan and the batch reader --------------------------------------------------------------------

// a BGZF file in memory: one member per text (an empty text: a member of ISIZE 0), the EOF member behind them when asked for
struct BgzfFile {
    std::vector<uint8_t> bytes;
    std::string text;
    std::vector<BgzfMember> mem;
    BgzfFile(const std::vector<std::string> &texts, bool eof)
    {
        for (const std::string &t : texts) {
            bgzf_member(reinterpret_cast<const uint8_t *>(t.data()), t.size(), 6, bytes);
            text += t;
        }
        if (eof) bytes.insert(bytes.end(), bgzf_eof_member(), bgzf_eof_member() + 28);
        index();
    }
    void index()
    {
        size_t total = 0;
        mem = bgzf_members(bytes.data(), bytes.size(), &total);
        CHECK(total == text.size());
    }
    // where member i starts, from the layout bgzf_member() writes (18 header bytes in front of the DEFLATE data)
    uint64_t start(size_t i) const { return mem[i].in_off - 18; }
};

// a few hundred bytes of text that no other call of it returns
std::string some_text(size_t n, unsigned seed)
{
    std::string t(n, '\0');
    for (size_t i = 0; i < n; i++) t[i] = "ACGTN\n@+IF"[((i + seed) * 2654435761u >> 9) % 10];
    return t;
}

const BgzfReadStyle kFastqStyle{no_room_device_error, ck_device_error, "compressed window", "inflated window", "member table"};
const BgzfReadStyle kBamStyle{bam_gpu_no_room, ck, "a batch of compressed bytes", nullptr, "the member table"};

// One pass of the reader over `f`: the text it hands over, batch by batch, held against the plan and the source.  resident: the
// batches land in one stream of the caller's.  Returns the count of members inflated on the host.
int64_t read_all(const BgzfFile &f, size_t batch, bool resident, bool timed = false)
{
    const BgzfBatchPlan plan = bgzf_batch_plan(f.mem, batch);
    std::vector<uint8_t> stream(f.text.size() + 64, 0xee);
    const std::vector<size_t> refuse = stub.refuse;
    stub.reset();
    stub.refuse = refuse;
    std::string got;
    size_t next_k = 0;
    const uint8_t *d_batch = nullptr;
    const BgzfReadStats st = read_bgzf_batches(ctx, resident ? kBamStyle : kFastqStyle, timed, f.bytes.data(), f.bytes.size(), f.mem, plan,
                                               resident ? stream.data() : nullptr, [&](const BgzfBatch &b) {
        if (b.k == 0) {                                                      // what the reader holds while it reads
            d_batch = b.d_text;
            if (resident) CHECK(stub.asked == (std::vector<size_t>{static_cast<size_t>(plan.max_in) + 64, MemberTable::kBytes}));
            else CHECK(stub.asked == (std::vector<size_t>{static_cast<size_t>(plan.max_in) + 64, static_cast<size_t>(plan.max_out) + 64, MemberTable::kBytes}));
            CHECK(stub.live.size() == stub.asked.size());
        }
        CHECK(b.k == next_k && b.k < plan.batches() && b.first == plan.cut[b.k] && b.n == plan.cut[b.k + 1] - b.first && b.n > 0);
        CHECK(b.in0 == f.start(b.first) && b.in1 == f.mem[b.first + b.n - 1].in_off + f.mem[b.first + b.n - 1].in_len + 8);
        CHECK(b.in1 - b.in0 <= plan.max_in && static_cast<uint64_t>(b.out_bytes) <= plan.max_out);
        CHECK(b.d_text == (resident ? stream.data() + f.mem[b.first].out_off : d_batch));
        CHECK(got.size() == f.mem[b.first].out_off);
        got.append(reinterpret_cast<const char *>(b.d_text), static_cast<size_t>(b.out_bytes));
        next_k++;
    });
    CHECK(next_k == plan.batches() && got == f.text);
    if (resident) CHECK(std::memcmp(stream.data(), f.text.data(), f.text.size()) == 0 && stream[f.text.size()] == 0xee);
    CHECK(stub.mallocs == (f.mem.empty() ? 0 : resident ? 2 : 3) && stub.syncs == (timed ? 3 * static_cast<int>(plan.batches()) : 0));     // (no member: no allocation)
    CHECK(st.upload >= 0 && st.inflate >= 0 && st.crc >= 0 && (timed || st.upload + st.inflate + st.crc == 0));
    const int64_t host = st.host_inflated;
    CHECK(stub.live.empty() && stub.bad_frees == 0);
    return host;
}

// the fault a pass over `f` ends with (kind, offset), or (-1, 0); everything the reader held is gone behind it
std::pair<int, uint64_t> fault_of(const BgzfFile &f, size_t batch, bool resident)
{
    const BgzfBatchPlan plan = bgzf_batch_plan(f.mem, batch);
    std::vector<uint8_t> stream(f.text.size() + 64);
    const std::vector<size_t> refuse = stub.refuse;
    stub.reset();
    stub.refuse = refuse;
    std::pair<int, uint64_t> got{-1, 0};
    try {
        read_bgzf_batches(ctx, kFastqStyle, false, f.bytes.data(), f.bytes.size(), f.mem, plan, resident ? stream.data() : nullptr, [](const BgzfBatch &) {});
    } catch (const BgzfMemberFault &e) { got = {static_cast<int>(e.kind), e.offset}; }
    CHECK(stub.live.empty() && stub.bad_frees == 0);
    return got;
}

std::vector<size_t> batch_sizes(size_t n)
{
    std::vector<size_t> b{1, 2, 3, n + 1};
    if (n > 3) b.push_back(n);
    return b;
}

void test_bgzf_plan()
{
    // every cut of 2 .. 9 members into batches of 1 .. 10, against sums over the members' own sizes
    for (size_t n = 2; n <= 9; n++) {
        std::vector<std::string> texts;
        for (size_t i = 0; i < n; i++) texts.push_back(i == n / 2 ? std::string() : some_text(40 + 97 * ((i * 5) % 7), static_cast<unsigned>(n * 16 + i)));
        const BgzfFile f(texts, false);
        CHECK(f.mem.size() == n);
        for (size_t i = 0; i < n; i++) CHECK(bgzf_member_start(f.mem, i) == f.start(i) && bgzf_member_end(f.mem, i) == (i + 1 < n ? f.start(i + 1) : f.bytes.size()));
        for (size_t batch = 1; batch <= 10; batch++) {
            std::vector<size_t> cut;
            std::vector<uint64_t> in((n + batch - 1) / batch, 0), out((n + batch - 1) / batch, 0);
            for (size_t i = 0; i < n; i++) {
                if (i % batch == 0) cut.push_back(i);
                in[i / batch] += 18 + f.mem[i].in_len + 8;
                out[i / batch] += f.mem[i].out_len;
            }
            cut.push_back(n);
            const BgzfBatchPlan plan = bgzf_batch_plan(f.mem, batch);
            CHECK(plan.cut == cut && plan.batches() == in.size());
            CHECK(plan.max_in == *std::max_element(in.begin(), in.end()) && plan.max_out == *std::max_element(out.begin(), out.end()));
        }
    }
    const BgzfBatchPlan none = bgzf_batch_plan({}, 3);                       // no member: no batch, nothing to hold
    CHECK(none.cut == std::vector<size_t>{0} && none.batches() == 0 && none.max_in == 0 && none.max_out == 0);
}

void test_bgzf_reader()
{
    const std::vector<std::string> five{some_text(300, 1), some_text(211, 2), some_text(640, 3), some_text(1, 4), some_text(455, 5)};
    std::vector<std::string> seven_texts = five;
    seven_texts.insert(seven_texts.begin() + 3, std::string());              // an empty member in the middle, the EOF member last: 7
    const BgzfFile none({}, false), one({some_text(333, 6)}, false), seven(seven_texts, true), no_eof({five[0], five[1], five[2], five[4]}, false);
    CHECK(none.mem.empty() && one.mem.size() == 1 && seven.mem.size() == 7 && seven.mem[3].out_len == 0 && seven.mem[6].out_len == 0 && no_eof.mem.size() == 4);
    CHECK(no_eof.mem.back().out_len != 0);
    for (const BgzfFile *f : {&none, &one, &seven, &no_eof})
        for (size_t batch : batch_sizes(f->mem.size()))
            for (bool resident : {false, true}) CHECK(read_all(*f, batch, resident) == 0);
    CHECK(read_all(seven, 2, false, true) == 0);                             // a timed run: three waits per batch
    CHECK(read_all(seven, 3, true, true) == 0);

    // members the device refuses, two of them empty: the host's decoder, the same text, three counted
    for (size_t batch : batch_sizes(7))
        for (bool resident : {false, true}) {
            stub.refuse = {0, 3, 6};
            CHECK(read_all(seven, batch, resident) == 3);
        }
    stub.refuse.clear();

    // a refused member that the host cannot inflate either; a member whose trailer states another CRC-32
    BgzfFile damaged = seven, wrong_crc = seven;
    damaged.bytes[damaged.mem[2].in_off] = 0x07;                             // (a last block of the reserved type)
    wrong_crc.bytes[wrong_crc.mem[4].in_off + wrong_crc.mem[4].in_len + 1] ^= 0x10;
    damaged.index();
    wrong_crc.index();
    for (size_t batch : batch_sizes(7))
        for (bool resident : {false, true}) {
            stub.refuse = {2};
            CHECK(fault_of(damaged, batch, resident) == std::make_pair(static_cast<int>(BgzfMemberFault::refused), damaged.start(2)));
            stub.refuse.clear();
            CHECK(fault_of(damaged, batch, resident) == std::make_pair(static_cast<int>(BgzfMemberFault::refused), damaged.start(2)));     // (refused by zlib too)
            CHECK(fault_of(wrong_crc, batch, resident) == std::make_pair(static_cast<int>(BgzfMemberFault::crc), wrong_crc.start(4)));
            CHECK(fault_of(seven, batch, resident) == std::make_pair(-1, uint64_t{0}));
        }
    CHECK(damaged.start(2) > 0 && wrong_crc.start(4) > damaged.start(2));

    // no room at each of the reader's allocations: the consumer's text and name, nothing left behind
    const BgzfBatchPlan plan = bgzf_batch_plan(seven.mem, 3);
    std::vector<uint8_t> stream(seven.text.size() + 64);
    for (bool resident : {false, true})
        for (int k = 1; k <= (resident ? 2 : 3); k++) {
            stub.reset();
            stub.fail_malloc = k;
            std::string said;
            try {
                read_bgzf_batches(ctx, resident ? kBamStyle : kFastqStyle, false, seven.bytes.data(), seven.bytes.size(), seven.mem, plan,
                                  resident ? stream.data() : nullptr, [](const BgzfBatch &) {});
            } catch (const DeviceNoRoom &e) { said = e.what(); }
            const char *name = resident ? (k == 1 ? kBamStyle.compressed : kBamStyle.table) : (k == 1 ? kFastqStyle.compressed : k == 2 ? kFastqStyle.inflated : kFastqStyle.table);
            const size_t bytes = k == (resident ? 2 : 3) ? MemberTable::kBytes : static_cast<size_t>(k == 1 ? plan.max_in : plan.max_out) + 64;
            CHECK(said == (resident ? kStyles[0] : kStyles[5]).want(std::to_string(bytes), name));
            CHECK(stub.mallocs == k && stub.live.empty() && stub.bad_frees == 0);
        }

    std::string said;                                                        // the failed call of fastq_gz.hpp / depth_read.hpp, in their words
    try { ck_device_error(-1, "member status"); } catch (const std::runtime_error &e) { said = e.what(); }
    CHECK(said == "device error (member status): out of memory (stub)");
    ck_device_error(0, "fine");
    const uint8_t four[4] = {0x78, 0x56, 0x34, 0x12};
    CHECK(le32(four) == 0x12345678u);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: device_scope_selftest <scratch directory>\n"); return 2; }
    test_scope();
    test_guards();
    test_clock();
    test_mapped_file(argv[1]);
    test_windows(argv[1]);
    test_paths_text();
    test_pending_outputs(argv[1]);
    test_duplicates();
    test_text_input(argv[1]);
    test_member_arithmetic();
    test_stored_member();
    test_bgzf_plan();
    test_bgzf_reader();
    std::printf("%s %d\n", failed ? "failed" : "ok", checks);
    return failed ? 1 : 0;
}
