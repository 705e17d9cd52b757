// The grammar of one region of `faidx <file.fa> region ...`, stated once: this one text is compiled by hipcc for the
// kernel of faidx.hip and by the host compiler for `faidx_region_selftest` (and its sanitizer build), so the device, the CPU tests
// and the sanitizer run check the same rules.
//   the whole string is a record's name        the whole record;
//   otherwise it is cut at its LAST ':'        the part in front must be a record's name, the part behind is the range:
//       B | B-E | B- | -E                      B, E: decimal digits in which ',' is ignored, at least one digit and at most 18;
//                                              1-based, inclusive; B = 0 counts as 1; a missing B is 1, a missing E the length.
//   E < B (B = 0 already counted as 1, E as written), a range of no bytes, a lone '-' and every other byte fail.  E beyond the
//   length is the length; B beyond the length gives no bases, which is no failure.
// Which record has a name is the caller's look-up: find(p, n) -> the record of the name p[0 .. n) or -1 (never found for n = 0),
// length(record) -> its bases.  Braces are not special.  No allocation, no library call, nothing of HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PALACE_FAIDX_FN __host__ __device__ __forceinline__
#else
#define PALACE_FAIDX_FN inline
#endif

namespace palace {

constexpr int kFaidxMaxDigits = 18;

// rec: the record, -1 for a region that fails; beg: the first base, 0-based; len: the bases, after clipping
struct FaidxRegion { int64_t rec, beg, len; };

// a number at p[i ..): digits and commas up to `end` or a byte that is neither.  False: no digit, or more than 18
PALACE_FAIDX_FN bool faidx_number(const uint8_t *p, int64_t &i, int64_t end, int64_t *value)
{
    int64_t v = 0;
    int digits = 0;
    for (; i < end; i++) {
        const uint32_t c = p[i];
        if (c == ',') continue;
        if (c < '0' || c > '9') break;
        if (++digits > kFaidxMaxDigits) return false;
        v = v * 10 + static_cast<int64_t>(c - '0');
    }
    *value = v;
    return digits > 0;
}

// the range p[0 .. n) behind the colon -> 1-based B and E as written (B = 0 already 1; a missing E: INT64_MAX).  False: no range
PALACE_FAIDX_FN bool faidx_range(const uint8_t *p, int64_t n, int64_t *b_out, int64_t *e_out)
{
    int64_t i = 0, b = 1, e = INT64_MAX;
    if (n <= 0) return false;
    if (p[0] == '-') {                                                       // -E
        i = 1;
        if (!faidx_number(p, i, n, &e) || i != n) return false;
    } else {
        if (!faidx_number(p, i, n, &b)) return false;
        if (b == 0) b = 1;
        if (i < n) {                                                         // B- or B-E
            if (p[i] != '-') return false;
            i++;
            if (i < n && (!faidx_number(p, i, n, &e) || i != n)) return false;
        }
    }
    if (e < b) return false;
    *b_out = b; *e_out = e;
    return true;
}

template <class Find, class Length>
PALACE_FAIDX_FN FaidxRegion faidx_region_resolve(const uint8_t *p, int64_t n, Find find, Length length)
{
    const FaidxRegion failed{-1, 0, 0};
    int64_t r = find(p, n);
    if (r >= 0) return FaidxRegion{r, 0, length(r)};
    int64_t colon = n - 1;
    while (colon >= 0 && p[colon] != ':') colon--;
    if (colon < 0) return failed;
    r = find(p, colon);
    if (r < 0) return failed;
    int64_t b, e;
    if (!faidx_range(p + colon + 1, n - colon - 1, &b, &e)) return failed;
    const int64_t len = length(r);
    if (b > len) return FaidxRegion{r, len, 0};
    if (e > len) e = len;
    return FaidxRegion{r, b - 1, e - (b - 1)};
}

}  // namespace palace
