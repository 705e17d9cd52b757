// `samtools depth` text in HBM -> totals and per-contig runs (include/palace_hip.h: palace_depth_parse): what `bamdepth --from-depth`
// needs to read a depth file back without its text crossing PCIe.  The grammar of a line is depth_line.hpp's.
//
// A window of text is three launches, count -> scan -> emit:
//   1. count: a tile of 4096 bytes (256 lanes x 16) finds its LFs by byte compares; a workgroup scan gives every LF its ordinal in
//      the tile; the lane that owns a line's LF parses the line from its end (depth_line_back) and compares its name with the bytes
//      behind the LF: a line whose successor has another name ENDS a run.  Per tile: lines, depth sum, first bad line, run ends and
//      the bytes of the names behind them -- those of the tile's last line kept apart, since only the scan knows whether a line
//      follows it in this window;
//   2. scan: one workgroup places every tile (first line, first run, first name byte), checks the capacities, moves the cursor
//      past the window (totals, first bad line, the unterminated tail for the next window), zeroes the window's runs and takes the
//      file's last line when it has no LF;
//   3. emit: every lane parses its lines again, now knowing their runs: depth sums are combined in the wavefront for the run the
//      wave starts in (one 64-bit atomic per wave when the whole wave lies in one run), the line behind a run end gathers its
//      name into d_names.
// The window's first line may begin in the cursor's tail (at most 4095 bytes): lines are read through a getter that has the tail
// in front of the window.  The cursor has two tail buffers: the scan writes the next window's while emit still reads this one's.
#include "common.hpp"
#include "depth_line.hpp"
#include "text_lanes.hpp"

namespace palace {
namespace {

constexpr int kTileThreads = 256, kTileBytes = kTileThreads * kLaneBytes;
constexpr int kScanThreads = 1024;
constexpr int64_t kMaxWindow = 1ll << 30;

static_assert(sizeof(palace_depth_cursor) == 64 + 2 * PALACE_DEPTH_TAIL_BYTES, "cursor layout");
static_assert(sizeof(palace_depth_run) == 24, "run layout");
static_assert(PALACE_DEPTH_TAIL_BYTES == kDepthLineMax, "the tail holds a line without its LF");

// per tile, by the count kernel.  ends / name_bytes: run ends among the tile's lines but the last, and the bytes of the names behind
// them; last_*: the same for the tile's last line; first_name_len: the name of the tile's first line (0: a bad line);
// first_bad: 1 + ordinal in the tile of its first bad line (0: none); last_lf: 1 + offset in the tile of its last LF
struct Tile { uint32_t nl, ends, name_bytes, last_end, last_name_len, first_name_len, first_bad, last_lf; uint64_t sum, pad; };
// per tile, by the scan kernel: ordinal of its first line in the window, run of that line, name bytes of the run ends in front of
// it; last_eff: a line follows the tile's last line in this window
struct TileBase { int64_t line0, run0, name0; int32_t last_eff, pad; };
struct ScratchHead { int32_t skip, tail_buf, tail_len, name0_len; int32_t pad[12]; };

inline size_t tiles_of(int64_t n) { return static_cast<size_t>((n + kTileBytes - 1) / kTileBytes); }

// the file's text around the window: byte i of the window for i >= 0, the carried tail at -tail_len .. -1
struct Text {
    const uint8_t *text, *tail;
    int64_t n;
    int32_t tail_len;
    __device__ __forceinline__ uint32_t operator()(int64_t i) const { return i < 0 ? tail[tail_len + i] : text[i]; }
};
__device__ __forceinline__ Text text_of(const uint8_t *text, int64_t n, const palace_depth_cursor *cur, int32_t buf, int32_t tail_len)
{
    tail_len = tail_len < 0 ? 0 : tail_len > kDepthLineMax - 1 ? kDepthLineMax - 1 : tail_len;
    return Text{text, cur->tail[buf & 1], n, tail_len};
}

// what a line means for the sums and the runs: good, depth, name; run_end: bytes follow its LF in the window and do not begin with
// its name and a TAB (a bad line always ends its run); next_len: then the length of the name that begins there (up to a TAB, an LF,
// the window's end or a line's length)
struct LineInfo { DepthLine d; bool run_end; int32_t next_len; };
__device__ __forceinline__ LineInfo line_at(const Text &t, int64_t e)
{
    LineInfo r{depth_line_back(t, -static_cast<int64_t>(t.tail_len), e), false, 0};
    const int64_t q = e + 1;
    if (q >= t.n) return r;
    bool same = r.d.error == kDepthLineOk && q + r.d.name_len < t.n;
    for (int32_t i = 0; same && i < r.d.name_len; i++) same = t(r.d.start + i) == t.text[q + i];
    if (same) same = t.text[q + r.d.name_len] == '\t';
    if (same) return r;
    r.run_end = true;
    const int64_t lim = q + kDepthLineMax - 1 < t.n ? q + kDepthLineMax - 1 : t.n;
    int64_t j = q;
    while (j < lim && t.text[j] != '\t' && t.text[j] != '\n') j++;
    r.next_len = static_cast<int32_t>(j - q);
    return r;
}

__global__ __launch_bounds__(kTileThreads) void depth_count_kernel(const uint8_t *text, int64_t n, const palace_depth_cursor *cur, Tile *tiles)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    __shared__ uint32_t s_pk, s_bad, s_first_len, s_last_end, s_last_len, s_last_lf;
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) { s_pk = 0; s_bad = ~0u; s_first_len = 0; s_last_end = 0; s_last_len = 0; s_last_lf = 0; s_sum = 0; }
    const Text t = text_of(text, n, cur, cur->tail_buf, cur->tail_len);
    const int64_t tile0 = static_cast<int64_t>(blockIdx.x) * kTileBytes, at = tile0 + threadIdx.x * kLaneBytes;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    uint32_t nlm = newline_mask(w, valid);
    uint32_t nl_total;
    uint32_t ord = block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(nlm)), s_scan, &nl_total);   // (syncs: the init above is seen)
    unsigned long long sum = 0;
    uint32_t pk = 0, bad = ~0u;
    for (; nlm; nlm &= nlm - 1, ord++) {
        const int64_t e = at + (__ffs(nlm) - 1);
        const LineInfo li = line_at(t, e);
        if (li.d.error == kDepthLineOk) sum += li.d.depth; else bad = bad < ord + 1 ? bad : ord + 1;
        if (ord == 0) s_first_len = static_cast<uint32_t>(li.d.name_len);
        if (ord == nl_total - 1) { s_last_end = li.run_end; s_last_len = static_cast<uint32_t>(li.next_len); s_last_lf = static_cast<uint32_t>(e - tile0) + 1; }
        else if (li.run_end) pk += 1u | (static_cast<uint32_t>(li.next_len) << 16);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64); pk += __shfl_xor(pk, d, 64);
        const uint32_t o = __shfl_xor(bad, d, 64);
        bad = bad < o ? bad : o;
    }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&s_sum, sum); atomicAdd(&s_pk, pk); atomicMin(&s_bad, bad); }
    __syncthreads();
    if (threadIdx.x == 0)
        tiles[blockIdx.x] = Tile{nl_total, s_pk & 0xffffu, s_pk >> 16, s_last_end, s_last_len, s_first_len, s_bad == ~0u ? 0u : s_bad, s_last_lf, s_sum, 0};
}

// one workgroup: the tiles' places, the capacities, the cursor moved past the window
__global__ __launch_bounds__(kScanThreads) void depth_scan_kernel(const uint8_t *text, int64_t n, int64_t n_tiles, int final_window,
                                                                  palace_depth_cursor *cur, const Tile *tiles, TileBase *bases, ScratchHead *head,
                                                                  palace_depth_run *runs, int64_t runs_cap, uint8_t *names, int64_t names_cap)
{
    __shared__ long long s_scan[kScanThreads / 64 + 1];
    __shared__ long long s_last_e, s_bad, s_runs, s_new_tail;
    __shared__ int s_name0, s_skip;
    const int64_t c_lines = cur->lines, c_bad = cur->bad_line;
    const uint64_t c_sum = cur->sum;
    const int32_t c_buf = cur->tail_buf & 1, c_error = cur->error;
    const Text t = text_of(text, n, cur, c_buf, cur->tail_len);
    if (threadIdx.x == 0) { s_last_e = -1; s_bad = INT64_MAX; s_name0 = 0; s_skip = 0; }
    __syncthreads();
    const int64_t per = (n_tiles + kScanThreads - 1) / kScanThreads;
    const int64_t t0 = threadIdx.x * per < n_tiles ? threadIdx.x * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    long long nl = 0, last_e = -1;
    for (int64_t k = t0; k < t1; k++) {
        nl += tiles[k].nl;
        if (tiles[k].nl) last_e = k * kTileBytes + tiles[k].last_lf - 1;
    }
    if (last_e >= 0) atomicMax(&s_last_e, last_e);
    long long nl_total;
    const long long line0 = block_exclusive<long long, kScanThreads>(nl, s_scan, &nl_total);
    const int64_t trailing = nl_total > 0 ? n - 1 - s_last_e : static_cast<int64_t>(t.tail_len) + n;   // bytes behind the last LF
    const bool tail_line = final_window && trailing > 0;
    const long long m = nl_total + (tail_line ? 1 : 0);                     // lines that end in this window
    long long ends = 0, name_bytes = 0, bad = INT64_MAX;
    unsigned long long sum = 0;
    {
        long long line = line0;
        for (int64_t k = t0; k < t1; k++) {
            const Tile tl = tiles[k];
            const bool eff = tl.nl && line + tl.nl < m && tl.last_end;
            ends += tl.ends + (eff ? 1 : 0); name_bytes += tl.name_bytes + (eff ? tl.last_name_len : 0);
            sum += tl.sum;
            if (tl.first_bad && bad == INT64_MAX) bad = c_lines + line + tl.first_bad;
            if (tl.nl && line == 0) s_name0 = static_cast<int>(tl.first_name_len);
            line += tl.nl;
        }
    }
    if (bad != INT64_MAX) atomicMin(&s_bad, bad);
    long long ends_total, bytes_total;
    unsigned long long sum_total;
    const long long run0 = block_exclusive<long long, kScanThreads>(ends, s_scan, &ends_total);
    const long long name0 = block_exclusive<long long, kScanThreads>(name_bytes, s_scan, &bytes_total);
    block_exclusive<unsigned long long, kScanThreads>(sum, reinterpret_cast<unsigned long long *>(s_scan), &sum_total);
    {
        long long line = line0, r = run0, b = name0;
        for (int64_t k = t0; k < t1; k++) {
            const Tile tl = tiles[k];
            const bool more = tl.nl && line + tl.nl < m;
            bases[k] = TileBase{line, r, b, more ? 1 : 0, 0};
            const bool eff = more && tl.last_end;
            r += tl.ends + (eff ? 1 : 0); b += tl.name_bytes + (eff ? tl.last_name_len : 0);
            line += tl.nl;
        }
    }
    // the file's last line, when it has no LF: one thread's
    DepthLine last{0, 0, 0u, 0u, kDepthLineOk};
    if (threadIdx.x == 0) {
        long long bad_line = s_bad;
        if (tail_line) {
            last = depth_line_back(t, -static_cast<int64_t>(t.tail_len), n);
            if (last.error == kDepthLineOk) sum_total += last.depth;
            else if (bad_line == INT64_MAX) bad_line = c_lines + m;
            if (nl_total == 0) s_name0 = last.name_len;
        }
        int64_t new_tail = final_window ? 0 : trailing;
        if (new_tail > kDepthLineMax - 1) {                                 // the line in progress is too long already
            if (bad_line == INT64_MAX) bad_line = c_lines + m + 1;
            new_tail = 0;
        }
        const int64_t n_runs = m > 0 ? 1 + ends_total : 0, n_names = (m > 0 ? s_name0 : 0) + bytes_total;
        cur->win_runs = n_runs; cur->win_name_bytes = n_names;              // (what the window needs, when it did not fit)
        if (c_error || n_runs > runs_cap || n_names > names_cap) {
            s_skip = 1;
            head->skip = 1;                                                 // nothing of this window is written
            cur->error = 1;
        } else {
            head->skip = 0; head->tail_buf = c_buf; head->tail_len = t.tail_len; head->name0_len = s_name0;
            cur->lines = c_lines + m;
            cur->sum = c_sum + sum_total;
            cur->bad_line = c_bad ? c_bad : bad_line == INT64_MAX ? 0 : bad_line;
            cur->tail_len = static_cast<int32_t>(new_tail);
            cur->tail_buf = c_buf ^ 1;
        }
        s_runs = n_runs; s_new_tail = new_tail;
    }
    __syncthreads();
    if (s_skip) return;
    for (int64_t k = threadIdx.x; k < s_runs; k += kScanThreads) runs[k] = palace_depth_run{0, 0, 0u, 0u};
    uint8_t *next_tail = cur->tail[c_buf ^ 1];
    for (int64_t k = threadIdx.x; k < s_new_tail; k += kScanThreads) next_tail[k] = static_cast<uint8_t>(t(n - s_new_tail + k));
    __syncthreads();
    if (threadIdx.x == 0 && tail_line) {
        palace_depth_run &r = runs[s_runs - 1];
        if (last.error == kDepthLineOk) { r.sum += last.depth; r.lines += 1; }
        if (nl_total == 0) {                                                // ... and the window's first: its run's name is its own
            r.name_off = 0; r.name_len = static_cast<uint32_t>(last.name_len);
            for (int32_t i = 0; i < last.name_len; i++) names[i] = static_cast<uint8_t>(t(last.start + i));
        }
    }
}

__global__ __launch_bounds__(kTileThreads) void depth_emit_kernel(const uint8_t *text, int64_t n, const palace_depth_cursor *cur, const TileBase *bases,
                                                                  const ScratchHead *head, palace_depth_run *runs, uint8_t *names)
{
    __shared__ uint32_t s_scan[kTileThreads / 64 + 1];
    if (head->skip) return;                                                  // (uniform)
    const Text t = text_of(text, n, cur, head->tail_buf, head->tail_len);
    const TileBase tb = bases[blockIdx.x];
    const int64_t at = static_cast<int64_t>(blockIdx.x) * kTileBytes + threadIdx.x * kLaneBytes;
    uint32_t w[4];
    const int valid = load_lane(text, n, at, w);
    const uint32_t nlm = newline_mask(w, valid);
    uint32_t nl_total, pk_total;
    const uint32_t ord0 = block_exclusive<uint32_t, kTileThreads>(static_cast<uint32_t>(__popc(nlm)), s_scan, &nl_total);
    // the lane's run ends (the tile's last line left out, as in the count kernel: nothing of the tile lies behind it)
    uint32_t pk = 0;
    {
        uint32_t ord = ord0;
        for (uint32_t m = nlm; m; m &= m - 1, ord++) {
            if (ord == nl_total - 1) break;
            const LineInfo li = line_at(t, at + (__ffs(m) - 1));
            if (li.run_end) pk += 1u | (static_cast<uint32_t>(li.next_len) << 16);
        }
    }
    const uint32_t before = block_exclusive<uint32_t, kTileThreads>(pk, s_scan, &pk_total);
    int64_t run = tb.run0 + (before & 0xffffu), name_at = static_cast<int64_t>(head->name0_len) + tb.name0 + (before >> 16);
    // the run the wave starts in: its sums are combined in the wave
    long long wave_run = nlm ? run : INT64_MAX;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(wave_run, d, 64);
        wave_run = wave_run < o ? wave_run : o;
    }
    unsigned long long acc_sum = 0, acc_lines = 0;
    {
        uint32_t ord = ord0;
        for (uint32_t m = nlm; m; m &= m - 1, ord++) {
            const int64_t e = at + (__ffs(m) - 1);
            const LineInfo li = line_at(t, e);
            if (li.d.error == kDepthLineOk) {
                if (run == wave_run) { acc_sum += li.d.depth; acc_lines++; }
                else {
                    atomicAdd(reinterpret_cast<unsigned long long *>(&runs[run].sum), static_cast<unsigned long long>(li.d.depth));
                    atomicAdd(reinterpret_cast<unsigned long long *>(&runs[run].lines), 1ull);
                }
            }
            if (tb.line0 + ord == 0) {                                      // the window's first line: run 0 is named by it
                runs[0].name_off = 0; runs[0].name_len = static_cast<uint32_t>(li.d.name_len);
                for (int32_t i = 0; i < li.d.name_len; i++) names[i] = static_cast<uint8_t>(t(li.d.start + i));
            }
            if (li.run_end && (ord != nl_total - 1 || tb.last_eff)) {       // the next line begins a run: its name
                run++;
                runs[run].name_off = static_cast<uint32_t>(name_at); runs[run].name_len = static_cast<uint32_t>(li.next_len);
                for (int32_t i = 0; i < li.next_len; i++) names[name_at + i] = text[e + 1 + i];
                name_at += li.next_len;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { acc_sum += __shfl_xor(acc_sum, d, 64); acc_lines += __shfl_xor(acc_lines, d, 64); }
    if ((threadIdx.x & 63) == 0 && acc_lines) {
        atomicAdd(reinterpret_cast<unsigned long long *>(&runs[wave_run].sum), acc_sum);
        atomicAdd(reinterpret_cast<unsigned long long *>(&runs[wave_run].lines), acc_lines);
    }
}

}  // namespace
}  // namespace palace

using namespace palace;

extern "C" size_t palace_depth_parse_scratch_bytes(int64_t max_window)
{
    const size_t t = tiles_of(max_window < 0 ? 0 : max_window);
    return align256(sizeof(ScratchHead)) + align256(t * sizeof(Tile)) + align256(t * sizeof(TileBase));
}

extern "C" int palace_depth_parse(palace_ctx *ctx, const uint8_t *d_text, int64_t n, int final_window, palace_depth_cursor *d_cursor,
                                  palace_depth_run *d_runs, int64_t runs_cap, uint8_t *d_names, int64_t names_cap, void *d_scratch,
                                  size_t scratch_bytes)
{
    PALACE_REQUIRE(ctx && n >= 0 && n <= kMaxWindow && runs_cap >= 0 && names_cap >= 0, "bad argument (a window has at most 2^30 bytes)");
    PALACE_REQUIRE(d_cursor && d_scratch && (d_runs || runs_cap == 0) && (d_names || names_cap == 0) && (d_text || n == 0), "null device pointer");
    PALACE_REQUIRE((reinterpret_cast<uintptr_t>(d_text) & 15) == 0, "the text must be 16-byte aligned");
    PALACE_REQUIRE(scratch_bytes >= palace_depth_parse_scratch_bytes(n), "scratch smaller than palace_depth_parse_scratch_bytes(n)");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    const size_t nt = tiles_of(n);
    uint8_t *s = static_cast<uint8_t *>(d_scratch);
    ScratchHead *head = reinterpret_cast<ScratchHead *>(s);
    Tile *tiles = reinterpret_cast<Tile *>(s + align256(sizeof(ScratchHead)));
    TileBase *tb = reinterpret_cast<TileBase *>(s + align256(sizeof(ScratchHead)) + align256(nt * sizeof(Tile)));
    if (nt) hipLaunchKernelGGL(depth_count_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, n, d_cursor, tiles);
    hipLaunchKernelGGL(depth_scan_kernel, dim3(1), dim3(kScanThreads), 0, ctx->stream, d_text, n, static_cast<int64_t>(nt), final_window, d_cursor,
                       tiles, tb, head, d_runs, runs_cap, d_names, names_cap);
    if (nt) hipLaunchKernelGGL(depth_emit_kernel, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, n, d_cursor, tb, head,
                               d_runs, d_names);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}
