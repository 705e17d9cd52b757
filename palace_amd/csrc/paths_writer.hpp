// Paths of tokens -> FASTA text, for the two tools that write one: make_fa_from_path (path_fasta.hip, PathsPolicy there) and
// make_final_fa (final_fasta.hip, FinalPolicy there).  A token is a record of the indexed assembly on either strand; a path's
// sequence is its tokens' bases one behind the other.  The scan of the tokens' sizes gives every token its place in the
// concatenation of all sequences (cum), the host gives every path its place in the output text (path_out); the writer maps an output
// byte to its path (window_lanes.hpp), to its token (searched once per lane in cum, then walked), to the base's place in the
// assembly's text.  See DESIGN.md 4 for the loads it issues.
//
// A policy states what differs:  Comp, the complement of a reversed token;  kSeparator, whether a token's size holds separator bytes
// in front of its bases (cum[t + 1] - cum[t] - the record's length of them, written as sep_byte);  kSkipEmptyPaths, whether a path
// without sequence has no text at all -- no header either -- so that its entry of path_out equals the next one and is passed over.
#pragma once
#include "window_lanes.hpp"

namespace palace {
namespace {

template <class Policy>
__global__ __launch_bounds__(kTileThreads) void paths_write_kernel(const uint8_t *text, const palace_fasta_rec *recs, const int32_t *code, const int64_t *cum,
                                                                   const int64_t *path_off, int64_t n_paths, const uint8_t *hdr, const int64_t *hdr_off,
                                                                   const int64_t *path_out, uint32_t sep_byte, int64_t lo, int64_t hi, uint8_t *out)
{
    __shared__ long long s_path[2];
    LaneOut l;
    int64_t p = window_lane(path_out, n_paths, lo, hi, s_path, &l);
    if (p < 0) return;
    while (!l.full()) {
        const int64_t h0 = hdr_off[p], h = hdr_off[p + 1] - h0, ta = path_off[p], tb = path_off[p + 1], base = cum[ta], len = cum[tb] - base;
        int64_t x = l.o0 + l.k - path_out[p];                                // the byte's place in the path's text
        put_header(l, hdr + h0, h, x);
        if (l.full()) break;
        int64_t q = x - (h + 2);                                             // ... in its sequence
        if (q < len) {
            int64_t t = last_le(cum, ta, tb - 1, base + q);                  // (behind tokens without bytes it is the last of equal entries)
            while (!l.full() && q < len) {
                while (cum[t + 1] <= base + q) t++;
                const int32_t c = code[t];
                const palace_fasta_rec r = recs[c >> 2];
                int64_t u = base + q - cum[t];                               // ... in its token's bytes
                if constexpr (Policy::kSeparator) {
                    const int64_t sep = cum[t + 1] - cum[t] - r.length;      // the separator's bytes come first
                    if (u < sep) {
                        const int64_t left = sep - u;
                        const int m = left < l.cnt - l.k ? static_cast<int>(left) : l.cnt - l.k;
                        for (int i = 0; i < m; i++) l.put(sep_byte);
                        q += m;
                        continue;
                    }
                    u -= sep;
                }
                const int64_t left = cum[t + 1] - base - q;
                const int m = left < l.cnt - l.k ? static_cast<int>(left) : l.cnt - l.k;
                if (gather_bases(l, text, r, u, m, (c & PALACE_PATH_REVERSE) != 0, out, typename Policy::Comp())) return;
                q += m;
            }
            if (l.full()) break;
        }
        l.put('\n');                                                         // the sequence's LF: the path is done
        if constexpr (Policy::kSkipEmptyPaths) do p++; while (p < n_paths - 1 && path_out[p + 1] == path_out[p]);
        else p++;
    }
    l.store(out);
}

// the checks behind an entry point's own first one, and the launch
template <class Policy>
int paths_write(const char *entry, palace_ctx *ctx, const uint8_t *d_text, const palace_fasta_rec *d_recs, const int32_t *d_code, const int64_t *d_tok_cum,
                const int64_t *d_path_off, int64_t n_paths, const uint8_t *d_hdr, const int64_t *d_hdr_off, const int64_t *d_path_out, uint32_t sep_byte,
                int64_t lo, int64_t hi, uint8_t *d_out)
{
    if (lo == hi) return PALACE_OK;
    PALACE_REQUIRE_AS(entry, n_paths > 0 && d_tok_cum && d_path_off && d_hdr_off && d_path_out && d_out, "null device pointer (or bytes asked of an empty text)");
    PALACE_REQUIRE_AS(entry, (reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "the output must be 16-byte aligned");
    const int64_t nt = (hi - lo + kTileBytes - 1) / kTileBytes;
    PALACE_REQUIRE_AS(entry, nt < (1ll << 31), "window too long");
    PALACE_HIP_TRY(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(paths_write_kernel<Policy>, dim3(static_cast<unsigned>(nt)), dim3(kTileThreads), 0, ctx->stream, d_text, d_recs, d_code, d_tok_cum, d_path_off,
                       n_paths, d_hdr, d_hdr_off, d_path_out, sep_byte, lo, hi, d_out);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

// ---- the tokens' places and the paths' lengths ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void path_len_kernel(const int64_t *cum, const int64_t *path_off, int64_t n_paths, int64_t *len)
{
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (p < n_paths) len[p] = cum[path_off[p + 1]] - cum[path_off[p]];
}

// d_tok_cum[0 .. n_tok]: the scan of size(token); d_path_len[p]: the bytes of path p's sequence.  ws_at: as scan_sizes'
template <class Size>
int paths_lengths(palace_ctx *ctx, Size size, int64_t n_tok, const int64_t *d_path_off, int64_t n_paths, int64_t *d_tok_cum, int64_t *d_path_len, size_t ws_at = 0)
{
    if (n_tok == 0) PALACE_HIP_TRY(hipMemsetAsync(d_tok_cum, 0, sizeof(int64_t), ctx->stream));
    else {
        const int rc = scan_sizes(ctx, size, n_tok, d_tok_cum, ws_at);
        if (rc) return rc;
    }
    if (n_paths)
        hipLaunchKernelGGL(path_len_kernel, dim3(static_cast<unsigned>((n_paths + 255) / 256)), dim3(256), 0, ctx->stream, d_tok_cum, d_path_off, n_paths, d_path_len);
    PALACE_HIP_TRY(hipGetLastError());
    return PALACE_OK;
}

}  // namespace
}  // namespace palace
