// The rules of `readqc` -- the driver's fastp call on a read pair (palace:358-363) -- stated once: the grammar of a FASTQ
// record, the overlap search of a pair, the trim it gives, the filter, and what the report counts.  This one text is compiled by
// hipcc for the kernels of readqc.hip -- where a wavefront owns a record or a pair and its lanes share the bytes and the candidates --
// and by the host compiler for host/fastq_rules_selftest_main.cpp, where the same pieces run one after the other.  fastp is not at
// hand, so these rules are the behaviour (parity UNPINNED).
//
// Every function is a pure function of its arguments: no allocation, no library call, nothing of HIP.
#pragma once
#include <cstdint>

#include "../../include/palace_hip.h"

#if defined(__HIPCC__)
#define PALACE_FQ_FN __device__ __forceinline__
#else
#define PALACE_FQ_FN inline
#endif

namespace palace {

// ---- the grammar ------------------------------------------------------------------------------------------------------------------
// A record is four lines: '@' name, SEQ, '+' anything, QUAL.  CR is a byte like any other, so it is a fault in SEQ and in QUAL.
PALACE_FQ_FN bool fastq_base_ok(uint32_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }
PALACE_FQ_FN bool fastq_qual_ok(uint32_t c) { return c >= 33 && c <= 126; }

// what a record's lines were found to be -> its first fault: the line within the record (0 .. 3) and the code; code 0: none
struct FastqFault { int32_t line, code; };
PALACE_FQ_FN FastqFault fastq_first_fault(bool no_at, bool too_long, bool bad_base, bool no_plus, bool qual_len, bool bad_qual)
{
    if (no_at) return FastqFault{0, PALACE_FASTQ_EAT};
    if (too_long) return FastqFault{1, PALACE_FASTQ_ELONG};
    if (bad_base) return FastqFault{1, PALACE_FASTQ_EBASE};
    if (no_plus) return FastqFault{2, PALACE_FASTQ_EPLUS};
    if (qual_len) return FastqFault{3, PALACE_FASTQ_EQLEN};
    if (bad_qual) return FastqFault{3, PALACE_FASTQ_EQUAL};
    return FastqFault{0, 0};
}

// the record whose line k is [b[k], e[k]), byte by byte (the kernel takes the bytes a lane each and ends in the same fastq_first_fault)
PALACE_FQ_FN FastqFault fastq_record_fault(const uint8_t *t, const int64_t b[4], const int64_t e[4])
{
    const int64_t l_seq = e[1] - b[1], l_qual = e[3] - b[3];
    const bool too_long = l_seq > PALACE_FASTQ_MAX_SEQ;
    bool bad_base = false, bad_qual = false;
    if (!too_long) {
        for (int64_t p = b[1]; p < e[1]; p++) bad_base |= !fastq_base_ok(t[p]);
        if (l_qual == l_seq)
            for (int64_t p = b[3]; p < e[3]; p++) bad_qual |= !fastq_qual_ok(t[p]);
    }
    return fastq_first_fault(e[0] == b[0] || t[b[0]] != '@', too_long, bad_base, e[2] == b[2] || t[b[2]] != '+', l_qual != l_seq, bad_qual);
}

// A whole text: cut at LF, a last line without LF is a line, the empty text has no line.  *records = complete records; the smallest
// faulty line (1-based) and its code, 0 / 0 for none.  Lines behind the last complete record are a record of fewer than 4 lines:
// PALACE_FASTQ_ELINES at its first line, its lines are not judged otherwise.
PALACE_FQ_FN void fastq_text_verdict(const uint8_t *t, int64_t n, int64_t *records, int64_t *bad_line, int32_t *code)
{
    *records = *bad_line = 0;
    *code = 0;
    int64_t b[4], e[4], at = 0, lines = 0;
    while (at < n) {
        int64_t end = at;
        while (end < n && t[end] != '\n') end++;
        b[lines & 3] = at; e[lines & 3] = end;
        lines++;
        at = end + 1;
        if ((lines & 3) == 0) {
            const FastqFault f = fastq_record_fault(t, b, e);
            if (f.code && !*code) { *bad_line = lines - 3 + f.line; *code = f.code; }
        }
    }
    *records = lines / 4;
    if ((lines & 3) && !*code) { *bad_line = 4 * (lines / 4) + 1; *code = PALACE_FASTQ_ELINES; }
}

// ---- the overlap of a pair -----------------------------------------------------------------------------------------------------------
// A: read 1's bases (L1).  B: the reverse complement of read 2's bases (L2).  Bytes are compared for equality, so N equals N.
PALACE_FQ_FN uint32_t fastq_complement(uint32_t c) { return c == 'A' ? 'T' : c == 'T' ? 'A' : c == 'C' ? 'G' : c == 'G' ? 'C' : c; }

// The candidates in search order: forward o = 0 .. F - 1 as (o, 0, min(L1 - o, L2)), then reverse k = 0 .. R - 1 as (0, k, min(L1, L2 - k)),
// F = max(0, L1 - require), R = max(0, L2 - require).
struct FastqCand { int32_t a0, b0, n; };
PALACE_FQ_FN int32_t fastq_forward_candidates(int32_t l1, const palace_readqc_params &p) { return l1 > p.overlap_require ? l1 - p.overlap_require : 0; }
PALACE_FQ_FN int32_t fastq_reverse_candidates(int32_t l2, const palace_readqc_params &p) { return l2 > p.overlap_require ? l2 - p.overlap_require : 0; }
PALACE_FQ_FN FastqCand fastq_candidate(int32_t c, int32_t l1, int32_t l2, const palace_readqc_params &p)
{
    const int32_t f = fastq_forward_candidates(l1, p);
    if (c < f) return FastqCand{c, 0, l1 - c < l2 ? l1 - c : l2};
    const int32_t k = c - f;
    return FastqCand{0, k, l1 < l2 - k ? l1 : l2 - k};
}
// accepted iff the mismatches among the first min(n, window) positions are <= min(diff_limit, n * diff_pct / 100)
PALACE_FQ_FN bool fastq_accept(const uint8_t *a, const uint8_t *b, FastqCand c, const palace_readqc_params &p)
{
    const int32_t pct = c.n * p.diff_pct / 100, limit = p.diff_limit < pct ? p.diff_limit : pct, m = c.n < p.diff_window ? c.n : p.diff_window;
    int32_t diff = 0;
    for (int32_t i = 0; i < m && diff <= limit; i++) diff += a[c.a0 + i] != b[c.b0 + i] ? 1 : 0;
    return diff <= limit;
}
// what the first accepted candidate (index c; -1: none) keeps of both reads: a reverse one with k >= 1 keeps n, everything else all
PALACE_FQ_FN int32_t fastq_trim_to(int32_t c, int32_t l1, int32_t l2, const palace_readqc_params &p)
{
    if (c < 0 || p.no_trim) return -1;
    const FastqCand x = fastq_candidate(c, l1, l2, p);
    return x.b0 >= 1 ? x.n : -1;
}

// ---- the filter ------------------------------------------------------------------------------------------------------------------------
// a read of l bases after trimming, `low` of its QUAL bytes below 33 + qual, n_n of its bases N -> 0 passes, else the reason
enum { kFastqPass = 0, kFastqLowQuality = 1, kFastqTooManyN = 2, kFastqTooShort = 3 };
PALACE_FQ_FN int32_t fastq_filter(int32_t l, int32_t low, int32_t n_n, const palace_readqc_params &p)
{
    if (!p.no_quality_filter) {
        if (static_cast<int64_t>(low) * 100 > static_cast<int64_t>(p.unqualified_percent) * l) return kFastqLowQuality;
        if (n_n > p.n_limit) return kFastqTooManyN;
    }
    if (!p.no_length_filter && l < p.min_length) return kFastqTooShort;
    return kFastqPass;
}
// a pair is kept iff both reads pass; a dropped pair counts under read 1's reason, or read 2's when read 1 passes
PALACE_FQ_FN int32_t fastq_pair_reason(int32_t r1, int32_t r2) { return r1 ? r1 : r2; }

// the bytes a kept pair's record takes in an output file: the name line, SEQ[0:n], line 2, QUAL[0:n], each with its LF
PALACE_FQ_FN int64_t fastq_record_bytes(int64_t name_len, int64_t plus_len, int64_t n) { return name_len + plus_len + 2 * n + 4; }

// ---- the report (readqc --full-report) --------------------------------------------------------------------------------------------------
// Written from fastp's stats.cpp and peprocessor.cpp as remembered; like the rest, these rules are the behaviour (parity UNPINNED).
// A base's slot in every per-cycle table: A C G T N = 0 .. 4 (the grammar admits nothing else).
enum { kFastqSlots = PALACE_READQC_SLOTS };
PALACE_FQ_FN int32_t fastq_base_slot(uint32_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4; }
// a QUAL byte's value, and whether it counts as Q20 / Q30
PALACE_FQ_FN uint32_t fastq_qual_value(uint32_t q) { return q - 33u; }
PALACE_FQ_FN bool fastq_is_q20(uint32_t q) { return q >= 33u + 20u; }
PALACE_FQ_FN bool fastq_is_q30(uint32_t q) { return q >= 33u + 30u; }

// The insert size of a pair from its first accepted candidate (index c; -1: none): a forward candidate at offset o >= 1 is a fragment
// longer than the overlap, L1 + L2 - n; at o = 0, and for every reverse candidate, the overlap is the fragment, n.  No candidate, and
// anything beyond the histogram, is slot PALACE_READQC_ISIZE_MAX: "unknown".
PALACE_FQ_FN int32_t fastq_insert_size(int32_t c, int32_t l1, int32_t l2, const palace_readqc_params &p)
{
    if (c < 0) return PALACE_READQC_ISIZE_MAX;
    const FastqCand x = fastq_candidate(c, l1, l2, p);
    const bool forward = c < fastq_forward_candidates(l1, p);
    const int32_t size = forward && x.a0 >= 1 ? l1 + l2 - x.n : x.n;
    return size > PALACE_READQC_ISIZE_MAX ? PALACE_READQC_ISIZE_MAX : size;
}

}  // namespace palace
