// Context, memory and timing plumbing of the C ABI (include/palace_hip.h).
#include "common.hpp"

#include <chrono>
#include <thread>

namespace palace {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

int ensure_workspace(palace_ctx *ctx, size_t bytes)
{
    if (ctx->ws.bytes >= bytes) return PALACE_OK;
    if (ctx->ws.ptr) {
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
        PALACE_HIP_TRY(hipFree(ctx->ws.ptr));
        ctx->ws.ptr = nullptr;
        ctx->ws.bytes = 0;
    }
    // the first request is taken as it is (a one-shot executable would only waste the head room); later growth adds 25 %
    size_t want = bytes + (ctx->ws_grown ? bytes / 4 : 0) + (1 << 20);
    ctx->ws_grown = true;
    hipError_t e = hipMalloc(&ctx->ws.ptr, want);
    if (e != hipSuccess) {
        set_error("workspace hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return PALACE_ENOMEM;
    }
    ctx->ws.bytes = want;
    return PALACE_OK;
}

int ensure_pinned(palace_ctx *ctx, size_t bytes)
{
    if (ctx->pin.bytes >= bytes) return PALACE_OK;
    if (ctx->pin.ptr) {
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
        PALACE_HIP_TRY(hipHostFree(ctx->pin.ptr));
        ctx->pin.ptr = nullptr;
        ctx->pin.bytes = 0;
    }
    const size_t want = bytes + bytes / 4 + (1 << 16);
    hipError_t e = hipHostMalloc(&ctx->pin.ptr, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("pinned staging hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        return PALACE_ENOMEM;
    }
    ctx->pin.bytes = want;
    return PALACE_OK;
}

int ensure_table(palace_ctx *ctx)
{
    for (int p = 0; p < 3; p++) {
        if (ctx->plane[p]) continue;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&ctx->plane[p]), kPlaneBytes);
        if (e != hipSuccess) {
            set_error("count-table plane hipMalloc failed: %s", hipGetErrorString(e));
            return PALACE_ENOMEM;
        }
        PALACE_HIP_TRY(hipMemsetAsync(ctx->plane[p], 0, kPlaneBytes, ctx->stream));
        if (p == 2) ctx->table.allocated_zeroed();
    }
    return PALACE_OK;
}

}  // namespace palace

using namespace palace;

extern "C" {

const char *palace_last_error(void) { return g_err; }
#ifndef PALACE_BUILD_ID
#define PALACE_BUILD_ID "unstamped"
#endif
const char *palace_version(void) { return "palace_hip 0.2 (gfx950) build " PALACE_BUILD_ID; }

int palace_ctx_create(int device, palace_ctx **out) { return palace_ctx_create_prio(device, 0, out); }

static int ctx_create(int device, int high_priority, hipStream_t given, palace_ctx **out);

int palace_ctx_create_prio(int device, int high_priority, palace_ctx **out)
{
    return ctx_create(device, high_priority, nullptr, out);
}

int palace_ctx_create_on_stream(int device, void *hip_stream, palace_ctx **out)
{
    PALACE_REQUIRE(hip_stream != nullptr, "stream is null");
    return ctx_create(device, 0, static_cast<hipStream_t>(hip_stream), out);
}

// (A stream confined to a set of compute units -- hipExtStreamCreateWithCUMask, palace_ctx_create_masked in rounds 4-5 -- was measured for
// stage 04 beside the counting kernels and never helped: what slows the small kernels is the memory system, not the CUs.  Removed in round 6.)
static int ctx_create(int device, int high_priority, hipStream_t given, palace_ctx **out)
{
    PALACE_REQUIRE(out != nullptr, "out is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error("no HIP device visible (%s)", e == hipSuccess ? "count is 0" : hipGetErrorString(e));
        return PALACE_EHIP;
    }
    PALACE_REQUIRE(device >= 0 && device < n, "device ordinal out of range");
    PALACE_HIP_TRY(hipSetDevice(device));
    palace_ctx *ctx = new palace_ctx();
    ctx->device = device;
    auto fail = [&](const char *what, hipError_t err) {      // nothing half-built is left behind
        set_error("%s failed: %s", what, hipGetErrorString(err));
        palace_ctx_destroy(ctx);
        return PALACE_EHIP;
    };
    if (given) {                                           // the caller's stream: used, never destroyed
        ctx->stream = given;
        ctx->owns_stream = false;
    } else if (high_priority) {
        int least = 0, greatest = 0;                       // numerically lower = more urgent
        if ((e = hipDeviceGetStreamPriorityRange(&least, &greatest)) != hipSuccess) return fail("hipDeviceGetStreamPriorityRange", e);
        if ((e = hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, greatest)) != hipSuccess) return fail("hipStreamCreateWithPriority", e);
    } else {
        if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) return fail("hipStreamCreateWithFlags", e);
    }
    if ((e = hipEventCreate(&ctx->ev0)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipEventCreate(&ctx->ev1)) != hipSuccess) return fail("hipEventCreate", e);
    if ((e = hipMalloc(reinterpret_cast<void **>(&ctx->d_small), 64 * sizeof(uint64_t))) != hipSuccess) return fail("hipMalloc", e);
    *out = ctx;
    return PALACE_OK;
}

int palace_ctx_destroy(palace_ctx *ctx)
{
    if (!ctx) return PALACE_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int p = 0; p < 3; p++)
        if (ctx->plane[p] && !ctx->planes_external) (void)hipFree(ctx->plane[p]);
    if (ctx->ws.ptr) (void)hipFree(ctx->ws.ptr);
    if (ctx->pin.ptr) (void)hipHostFree(ctx->pin.ptr);
    if (ctx->match_scratch) palace::free_match_scratch(ctx->match_scratch);
    if (ctx->d_small) (void)hipFree(ctx->d_small);
    for (hipEvent_t e : ctx->marks)
        if (e) (void)hipEventDestroy(e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->stream && ctx->owns_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PALACE_OK;
}

int palace_sync(palace_ctx *ctx)
{
    PALACE_REQUIRE(ctx, "ctx is null");
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PALACE_OK;
}

void *palace_stream(palace_ctx *ctx) { return ctx ? ctx->stream : nullptr; }

int palace_malloc(palace_ctx *ctx, size_t bytes, void **d_out)
{
    PALACE_REQUIRE(ctx && d_out, "null argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(d_out, bytes ? bytes : 1);
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return PALACE_ENOMEM;
    }
    return PALACE_OK;
}

int palace_free(palace_ctx *ctx, void *d_ptr)
{
    PALACE_REQUIRE(ctx, "ctx is null");
    if (!d_ptr) return PALACE_OK;
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    PALACE_HIP_TRY(hipFree(d_ptr));
    return PALACE_OK;
}

int palace_memset(palace_ctx *ctx, void *d_ptr, int value, size_t bytes)
{
    PALACE_REQUIRE(ctx && (d_ptr || !bytes), "null argument");
    if (bytes) PALACE_HIP_TRY(hipMemsetAsync(d_ptr, value, bytes, ctx->stream));
    return PALACE_OK;
}

int palace_h2d(palace_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    PALACE_REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), "null argument");
    if (bytes) {
        PALACE_HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));   // h_src may be pageable
    }
    return PALACE_OK;
}

int palace_host_alloc(palace_ctx *ctx, size_t bytes, void **h_out)
{
    PALACE_REQUIRE(ctx && h_out, "null argument");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipError_t e = hipHostMalloc(h_out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        return PALACE_ENOMEM;
    }
    return PALACE_OK;
}

int palace_host_free(palace_ctx *ctx, void *h_ptr)
{
    PALACE_REQUIRE(ctx, "ctx is null");
    if (!h_ptr) return PALACE_OK;
    PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    PALACE_HIP_TRY(hipHostFree(h_ptr));
    return PALACE_OK;
}

int palace_h2d_async(palace_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    PALACE_REQUIRE(ctx && (bytes == 0 || (d_dst && h_src)), "null argument");
    if (bytes) PALACE_HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return PALACE_OK;
}

int palace_d2h_async(palace_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    PALACE_REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), "null argument");
    if (bytes) PALACE_HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return PALACE_OK;
}

int palace_mark_wait(palace_ctx *ctx, int i)
{
    PALACE_REQUIRE(ctx && i >= 0 && static_cast<size_t>(i) < ctx->marks.size() && ctx->marks[i], "mark not recorded");
    PALACE_HIP_TRY(hipEventSynchronize(ctx->marks[i]));
    return PALACE_OK;
}

int palace_mark_wait_for(palace_ctx *ctx, int i, double seconds)
{
    PALACE_REQUIRE(ctx && i >= 0 && static_cast<size_t>(i) < ctx->marks.size() && ctx->marks[i], "mark not recorded");
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ctx->marks[i]);
        if (e == hipSuccess) return PALACE_OK;
        if (e != hipErrorNotReady) { set_error("hipEventQuery failed: %s", hipGetErrorString(e)); return PALACE_EHIP; }
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > seconds) {
            set_error("palace_mark_wait_for: mark %d not reached after %.1f s", i, seconds);
            return PALACE_ESTATE;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

int palace_d2h(palace_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    PALACE_REQUIRE(ctx && (bytes == 0 || (h_dst && d_src)), "null argument");
    if (bytes) {
        PALACE_HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
        PALACE_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return PALACE_OK;
}

int palace_d2d(palace_ctx *ctx, void *d_dst, const void *d_src, size_t bytes)
{
    PALACE_REQUIRE(ctx && (bytes == 0 || (d_dst && d_src)), "null argument");
    if (bytes) PALACE_HIP_TRY(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return PALACE_OK;
}

int palace_timer_begin(palace_ctx *ctx)
{
    PALACE_REQUIRE(ctx, "ctx is null");
    PALACE_HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return PALACE_OK;
}

int palace_timer_end(palace_ctx *ctx, float *ms_out)
{
    PALACE_REQUIRE(ctx && ms_out, "null argument");
    PALACE_HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    PALACE_HIP_TRY(hipEventSynchronize(ctx->ev1));
    PALACE_HIP_TRY(hipEventElapsedTime(ms_out, ctx->ev0, ctx->ev1));
    return PALACE_OK;
}

int palace_mark(palace_ctx *ctx, int i)
{
    PALACE_REQUIRE(ctx && i >= 0 && i < 4096, "mark index out of range");
    if (ctx->marks.size() <= static_cast<size_t>(i)) ctx->marks.resize(i + 1, nullptr);
    if (!ctx->marks[i]) PALACE_HIP_TRY(hipEventCreate(&ctx->marks[i]));
    PALACE_HIP_TRY(hipEventRecord(ctx->marks[i], ctx->stream));
    return PALACE_OK;
}

int palace_wait_for_mark(palace_ctx *ctx, palace_ctx *other, int i)
{
    PALACE_REQUIRE(ctx && other && i >= 0 && static_cast<size_t>(i) < other->marks.size() && other->marks[i], "mark not recorded");
    PALACE_HIP_TRY(hipStreamWaitEvent(ctx->stream, other->marks[i], 0));
    return PALACE_OK;
}

int palace_mark_elapsed(palace_ctx *ctx, int a, int b, float *ms_out)
{
    PALACE_REQUIRE(ctx && ms_out && a >= 0 && b >= 0 && static_cast<size_t>(a) < ctx->marks.size() &&
                       static_cast<size_t>(b) < ctx->marks.size() && ctx->marks[a] && ctx->marks[b],
                   "marks not recorded");
    PALACE_HIP_TRY(hipEventSynchronize(ctx->marks[b]));
    PALACE_HIP_TRY(hipEventElapsedTime(ms_out, ctx->marks[a], ctx->marks[b]));
    return PALACE_OK;
}

}  // extern "C"
