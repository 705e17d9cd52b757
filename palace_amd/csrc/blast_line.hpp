// The grammar of one line of the BLAST table that filter_result reads (`-outfmt 6`), stated once: this one text is
// compiled by hipcc for the kernels of filter_result.hip and by the host compiler for `blast_line_selftest` (and its sanitizer
// build), so the device, the CPU tests and the sanitizer run check the same rules.
//   the line    at least four columns, cut at TAB (the LF is not part of it; no byte is stripped);
//   column 0    the query: 1 or more bytes (that it is a record of the FASTA is the caller's look-up);
//   column 1    the subject: 1 or more bytes;
//   column 2    the identity, `digits[.digits]`: 1-3 digits, then nothing or a point and 1-6 digits.  It is READ as the integer its
//               digits spell, with k = 0 .. 6 decimals: the text stands for exactly value / 10^k;
//   column 3    the alignment length: 1-10 digits;
//   the rest    is not looked at.
// No sign, no exponent, no space, no CR in the four columns.  There is no text-to-float here: `float(column 2) > cut` is
// value >= cut[k], where cut[k] is the smallest integer N with (double)N / 10^k > cut -- blast_identity_cuts finds it by bisection
// over correctly rounded divisions, and float() of the text is the correctly rounded quotient of the same two integers.
// No allocation, no library call, nothing of HIP.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PALACE_BLAST_FN __host__ __device__ __forceinline__
#else
#define PALACE_BLAST_FN inline
#endif

namespace palace {

constexpr int kBlastCuts = 7;                        // k = 0 .. 6 decimals

enum BlastLineError : int32_t {
    kBlastLineOk = 0,
    kBlastLineColumns = 1,     // fewer than four columns
    kBlastLineEmptyName = 2,   // an empty query or subject
    kBlastLineIdentity = 3,    // column 2 is not digits[.digits] with at most 3 and 6 digits
    kBlastLineLength = 4,      // column 3 is not 1-10 digits
    kBlastLineQuery = 5,       // the query is no record of the FASTA (the caller's look-up)
    kBlastLineQueryEmpty = 6   // the query's record has no bases
};

struct BlastLine {
    int64_t ident;          // column 2's digits as an integer
    int32_t decimals;       // how many of them stand behind the point
    int64_t length;         // column 3
    int32_t error;          // BlastLineError 0 .. 4; the fields above hold nothing when it is not kBlastLineOk
};

// The line [b, e) of a text whose byte i is get(i), its first tabs already found: c[k] = the index behind the k-th TAB for
// k = 1 .. min(tabs, 4), tabs = the TABs of the line counted up to 4 at least (a larger count is as good as 4).
template <class Get>
PALACE_BLAST_FN BlastLine blast_line_fields(Get get, int64_t b, int64_t e, const int64_t *c, int64_t tabs)
{
    BlastLine r{0, 0, 0, kBlastLineOk};
    if (tabs < 3) { r.error = kBlastLineColumns; return r; }
    if (c[1] - 1 == b || c[2] - 1 == c[1]) { r.error = kBlastLineEmptyName; return r; }
    {
        int64_t i = c[2];
        const int64_t end = c[3] - 1;
        int digits = 0;
        while (i < end && get(i) >= '0' && get(i) <= '9' && digits < 3) { r.ident = r.ident * 10 + (get(i) - '0'); i++; digits++; }
        bool ok = digits > 0;
        if (ok && i < end) {
            ok = get(i) == '.';
            i++;
            while (ok && i < end && get(i) >= '0' && get(i) <= '9' && r.decimals < 6) { r.ident = r.ident * 10 + (get(i) - '0'); i++; r.decimals++; }
            ok = ok && r.decimals > 0 && i == end;
        }
        if (!ok) { r.error = kBlastLineIdentity; return r; }
    }
    {
        int64_t i = c[3];
        const int64_t end = tabs >= 4 ? c[4] - 1 : e;
        int digits = 0;
        while (i < end && get(i) >= '0' && get(i) <= '9' && digits < 10) { r.length = r.length * 10 + (get(i) - '0'); i++; digits++; }
        if (digits == 0 || i != end) { r.error = kBlastLineLength; return r; }
    }
    return r;
}

// a line held in memory: p[0 .. len), no LF inside
PALACE_BLAST_FN BlastLine blast_line_parse(const uint8_t *p, int64_t len)
{
    int64_t c[5] = {0, 0, 0, 0, 0}, tabs = 0;
    for (int64_t i = 0; i < len && tabs < 4; i++)
        if (p[i] == '\t') c[++tabs] = i + 1;
    return blast_line_fields([p](int64_t i) { return static_cast<uint32_t>(p[i]); }, 0, len, c, tabs);
}

// whether the line's identity passes `float(column 2) > cut` for the cuts blast_identity_cuts made of `cut`
PALACE_BLAST_FN bool blast_identity_passes(const BlastLine &l, const int64_t *cut) { return l.ident >= cut[l.decimals]; }

// cut[k], k = 0 .. 6: the smallest integer N in [0, 10^(3 + k)] with (double)N / 10^k > threshold, 10^(3 + k) -- above every value
// the grammar can spell -- when there is none (a NaN threshold too).  The quotient does not fall as N grows, so bisection finds it.
inline void blast_identity_cuts(double threshold, int64_t *cut)
{
    int64_t p10 = 1;
    for (int k = 0; k < kBlastCuts; k++, p10 *= 10) {
        int64_t lo = 0, hi = 1000 * p10;             // the answer is in [lo, hi]
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (static_cast<double>(mid) / static_cast<double>(p10) > threshold) hi = mid; else lo = mid + 1;
        }
        cut[k] = lo;
    }
}

inline const char *blast_line_error_text(int32_t e)
{
    switch (e) {
    case kBlastLineOk: return "ok";
    case kBlastLineColumns: return "fewer than four columns";
    case kBlastLineEmptyName: return "an empty query or subject";
    case kBlastLineIdentity: return "an identity that is not digits[.digits] with at most 3 and 6 digits";
    case kBlastLineLength: return "an alignment length that is not 1-10 digits";
    case kBlastLineQuery: return "the query is no record of the FASTA";
    default: return "the query's record has no bases";
    }
}

}  // namespace palace
