// The rules of one BAM alignment record, stated once: the step of the record walk, the size of an aux value, the CIGAR a record
// really has, its spans, clips and match segments, the first NM and SA fields, the read name's key, and the SA text's items.  This
// one text is compiled by hipcc for the kernels of bam.hip and by the host compiler for the loader of host/bam.cpp, so the two
// cannot disagree; what differs between them -- how the stream gets there, who walks it, how a contig name is looked up -- stays
// with each side.  Stands in for what htslib does inside sam_read1 / bam_aux_get and for parseSAItem / parseCigarReadInterval of
// the reference (generate_graph.cpp:185-206, 330-397, 644-698); written against the SAM/BAM specification.
//
// Every function is a pure function of the inflated stream `d` and offsets into it (the stream has no alignment anywhere): no
// allocation, no library call, nothing of HIP.  A record is named by `s`, the offset of its refID (its size word lies at s - 4);
// `end` is the offset behind it.  Every read lies inside the record the walk accepted.  Lengths are summed in uint32_t, as the
// wrap of 2^32 is defined, and cast where they are stored.
#pragma once
#include <cstdint>

#include "../../include/palace_hip.h"

#if defined(__HIPCC__)
#define PALACE_BAM_FN __device__ __forceinline__
#define PALACE_BAM_UNROLL _Pragma("unroll")
#else
#define PALACE_BAM_FN inline
#define PALACE_BAM_UNROLL
#endif

namespace palace {

PALACE_BAM_FN uint32_t ld16(const uint8_t *d, int64_t p) { return d[p] | (static_cast<uint32_t>(d[p + 1]) << 8); }
PALACE_BAM_FN uint32_t ld32(const uint8_t *d, int64_t p)
{
    return d[p] | (static_cast<uint32_t>(d[p + 1]) << 8) | (static_cast<uint32_t>(d[p + 2]) << 16) | (static_cast<uint32_t>(d[p + 3]) << 24);
}

// One step of THE walk at offset p, on the bytes [0, limit) of a stream of `total` bytes: 1 = a record (*next = the offset behind
// it), 0 = the stream ends or is malformed here (the walk is over), -1 = not decidable on `limit` bytes yet (a caller that has the
// whole stream passes limit == total and never sees it).  The only place the record rules live.
PALACE_BAM_FN int walk_step(const uint8_t *d, int64_t p, int64_t limit, int64_t total, int64_t *next)
{
    if (p + 4 > total) return 0;
    if (p + 4 > limit) return -1;
    const int64_t bs = ld32(d, p);
    if (bs < 32) return 0;                                                   // truncated tail: stop like a failed sam_read1
    if (p + 4 + bs > total) return 0;
    if (p + 4 + bs > limit) return -1;
    // the variable-length fields must fit the record (htslib's bam_read1 fails on such a record, which ends the reference's
    // `while (sam_read1(...) >= 0)` loop at generate_graph.cpp:644): name, CIGAR, packed bases, qualities
    const int64_t r = p + 4;
    const int64_t l_name = d[r + 8], n_cig = ld16(d, r + 12), l_seq = ld32(d, r + 16);
    if (l_name < 1 || l_seq > 0x7fffffffll || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) return 0;
    *next = p + 4 + bs;
    return 1;
}

// size of one aux value at v (type byte consumed); 0 = unknown type or malformed
PALACE_BAM_FN uint64_t aux_size(const uint8_t *d, uint32_t type, int64_t v, int64_t end)
{
    switch (type) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    case 'Z': case 'H':
        for (int64_t q = v; q < end; q++)
            if (d[q] == 0) return static_cast<uint64_t>(q - v + 1);
        return 0;
    case 'B': {                                                              // subtype, int32 count, count elements
        if (end - v < 5) return 0;
        uint64_t es;
        switch (d[v]) {
        case 'c': case 'C': es = 1; break;
        case 's': case 'S': es = 2; break;
        case 'i': case 'I': case 'f': es = 4; break;
        default: return 0;
        }
        return 5 + es * static_cast<uint64_t>(ld32(d, v + 1));
    }
    default: return 0;
    }
}

// The record's CIGAR as the reference sees it: its own ops, or the first CG:B,I tag's behind the <l_seq>S<ref>N placeholder of a
// mapped record (a CIGAR of more than 65535 ops, SAM spec 4.2.2; htslib puts it back in place inside bam_read1).  ops = offset of
// the first op word, aux = offset of the first aux field.
struct RecCigar { int64_t ops, n_ops, aux; };
PALACE_BAM_FN RecCigar record_cigar(const uint8_t *d, int64_t s, int64_t end)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s)), pos = static_cast<int32_t>(ld32(d, s + 4));
    const int64_t l_name = d[s + 8], n_cig = ld16(d, s + 12), l_seq = ld32(d, s + 16);
    const int64_t cg = s + 32 + l_name;
    RecCigar c{cg, n_cig, cg + 4 * n_cig + (l_seq + 1) / 2 + l_seq};
    if (n_cig > 0 && tid >= 0 && pos >= 0 && (ld32(d, cg) & 15u) == 4 && static_cast<int64_t>(ld32(d, cg) >> 4) == l_seq) {
        for (int64_t x = c.aux; x + 3 <= end;) {
            const int64_t v = x + 3;
            const uint32_t type = d[x + 2];
            const uint64_t sz = aux_size(d, type, v, end);
            if (!sz || sz > static_cast<uint64_t>(end - v)) break;
            if (d[x] == 'C' && d[x + 1] == 'G') {                            // the first CG tag decides (bam_aux_get)
                if (type == 'B' && (d[v] == 'I' || d[v] == 'i') && ld32(d, v + 1) >= static_cast<uint32_t>(n_cig) && ld32(d, v + 1) < (1u << 29)) {
                    c.ops = v + 5;
                    c.n_ops = ld32(d, v + 1);
                }
                break;
            }
            x = v + static_cast<int64_t>(sz);
        }
    }
    return c;
}

// One CIGAR as parseCigarReadInterval sees it (generate_graph.cpp:330-366): zero-length ops are dropped; the leading S, the
// trailing S when more than one op remains, len = the query span
struct OpScan {
    int32_t n_ops = 0, first_len = 0, last_len = 0;
    bool first_s = false, last_s = false;
    uint32_t len = 0;
    PALACE_BAM_FN void add(int32_t n, bool is_s, bool in_read)
    {
        if (n <= 0) return;
        if (!n_ops) { first_s = is_s; first_len = n; }
        last_s = is_s; last_len = n; n_ops++;
        if (in_read) len += static_cast<uint32_t>(n);
    }
    PALACE_BAM_FN int32_t clip_s() const { return n_ops && first_s ? first_len : 0; }
    PALACE_BAM_FN int32_t clip_e() const { return n_ops > 1 && last_s ? last_len : 0; }
};

// what `samtools depth` counts: UNMAP, SECONDARY, QCFAIL and DUP clear, on a contig of the header, at a position
PALACE_BAM_FN bool depth_counts(const uint8_t *d, int64_t s, int32_t n_ref)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s)), pos = static_cast<int32_t>(ld32(d, s + 4));
    return !(ld16(d, s + 14) & 0x704u) && tid >= 0 && tid < n_ref && pos >= 0;
}

// The op loop: ref_len (bam_cigar2rlen), read_len (getReadLength, :385-397), the clips, and -- when `segments` -- f(tid, pos, len)
// for every M / = / X operation of a length, at pos + (reference consumed so far), in operation order
struct RecOps { uint32_t ref_len = 0, read_len = 0; OpScan sc; };
template <class F>
PALACE_BAM_FN RecOps record_ops(const uint8_t *d, int64_t s, const RecCigar &c, bool segments, F f)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s));
    const uint32_t pos = ld32(d, s + 4);
    RecOps r;
    for (int64_t k = 0; k < c.n_ops; k++) {
        const uint32_t w = ld32(d, c.ops + 4 * k), op = w & 15u, len = w >> 4;
        const bool in_read = op == 0 || op == 1 || op == 4 || op == 7 || op == 8;
        if (segments && len > 0 && (op == 0 || op == 7 || op == 8)) f(tid, static_cast<int32_t>(pos + r.ref_len), static_cast<int32_t>(len));
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) r.ref_len += len;
        if (in_read) r.read_len += len;
        r.sc.add(static_cast<int32_t>(len), op == 4, in_read);
    }
    return r;
}

// f(tid, pos, len) for every match segment of the record, none for a record that depth does not count
template <class F>
PALACE_BAM_FN void record_segments(const uint8_t *d, int64_t s, int32_t n_ref, F f)
{
    if (!depth_counts(d, s, n_ref)) return;
    record_ops(d, s, record_cigar(d, s, s + static_cast<int64_t>(ld32(d, s - 4))), true, f);
}

// The coordinate-sort key of a record in a file of n_ref targets (the order of samtools' bam1_cmp_core): the contig, records without
// one last; then pos + 1, so that pos = -1 comes first; then the strand bit, forward first.  31 + 32 + 1 bits.  sort_key_ok: the
// record has a key at all (refID in [-1, n_ref), pos >= -1).
PALACE_BAM_FN bool sort_key_ok(const uint8_t *d, int64_t s, int32_t n_ref)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s)), pos = static_cast<int32_t>(ld32(d, s + 4));
    return tid >= -1 && tid < n_ref && pos >= -1;
}
PALACE_BAM_FN uint64_t sort_key(const uint8_t *d, int64_t s, int32_t n_ref)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s));
    const uint64_t t = static_cast<uint32_t>(tid < 0 ? n_ref : tid);
    return t << 33 | static_cast<uint64_t>(ld32(d, s + 4) + 1u) << 1 | (ld16(d, s + 14) >> 4 & 1u);
}

// reg2bin of the SAM specification 5.3 for the interval [beg, end), 0 <= beg < end <= 2^29
PALACE_BAM_FN uint32_t reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return static_cast<uint32_t>(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return static_cast<uint32_t>(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return static_cast<uint32_t>(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return static_cast<uint32_t>(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return static_cast<uint32_t>(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// The interval a .bai files a record under: [pos, pos + ref_len) of the CIGAR the record really has (record_cigar: the CG tag's
// N already carries the placeholder's span), one base for an unmapped record (flag 0x4), one without ops or without reference bases.
// ok: a .bai can hold it (pos >= 0, end <= 2^29).  Asked only of records with refID >= 0.
struct BaiSpan { int64_t beg, end; bool ok; };
PALACE_BAM_FN BaiSpan bai_span(const uint8_t *d, int64_t s)
{
    const int64_t beg = static_cast<int32_t>(ld32(d, s + 4));
    int64_t len = 0;
    if (!(ld16(d, s + 14) & 4u)) {
        const RecCigar c = record_cigar(d, s, s + static_cast<int64_t>(ld32(d, s - 4)));
        len = record_ops(d, s, c, false, [](int32_t, int32_t, int32_t) {}).ref_len;
    }
    const int64_t end = beg + (len > 0 ? len : 1);
    return BaiSpan{beg, end, beg >= 0 && end <= (1ll << 29)};
}

// the C-string view of the read name (:651): up to the first NUL inside l_read_name, else l_read_name - 1 bytes (l_read_name >= 1: the walk)
PALACE_BAM_FN int64_t name_len(const uint8_t *d, int64_t s)
{
    const int64_t l_name = d[s + 8];
    for (int64_t k = 0; k < l_name; k++)
        if (d[s + 32 + k] == 0) return k;
    return l_name - 1;
}

// 64-bit key of the n name bytes at `at` (seeded so that a collision can be escaped by re-keying)
PALACE_BAM_FN uint64_t name_key(const uint8_t *d, int64_t at, int64_t n, uint64_t seed)
{
    uint64_t h = 0xcbf29ce484222325ull ^ (seed * 0x9e3779b97f4a7c15ull);
    for (int64_t i = 0; i < n; i++) { h ^= d[at + i]; h *= 0x100000001b3ull; }
    h ^= h >> 32; h *= 0xd6e8feb86659fd93ull; h ^= h >> 32;
    return h;
}

// The aux scan from x0: the first NM field decides nm (integer types with their signedness, like bam_aux2i; any other type 0), the
// first SA field of type Z is the SA text [sa, sa + sa_len) (sa = -1: none); the scan stops at a field of unknown size or past the
// record, and once both are found
struct RecAux { int32_t nm; int64_t sa, sa_len; };
PALACE_BAM_FN RecAux record_aux(const uint8_t *d, int64_t x0, int64_t end)
{
    RecAux a{0, -1, 0};
    bool have_nm = false, have_sa = false;
    for (int64_t x = x0; x + 3 <= end && !(have_nm && have_sa);) {
        const int64_t v = x + 3;
        const uint32_t type = d[x + 2];
        const uint64_t sz = aux_size(d, type, v, end);
        if (!sz || sz > static_cast<uint64_t>(end - v)) break;
        if (!have_nm && d[x] == 'N' && d[x + 1] == 'M') {
            have_nm = true;
            switch (type) {
            case 'c': a.nm = static_cast<int8_t>(d[v]); break;
            case 'C': a.nm = d[v]; break;
            case 's': a.nm = static_cast<int16_t>(ld16(d, v)); break;
            case 'S': a.nm = static_cast<int32_t>(ld16(d, v)); break;
            case 'i': case 'I': a.nm = static_cast<int32_t>(ld32(d, v)); break;
            default: a.nm = 0;
            }
        } else if (!have_sa && d[x] == 'S' && d[x + 1] == 'A' && type == 'Z') {
            have_sa = true;
            a.sa = v;
            a.sa_len = static_cast<int64_t>(sz) - 1;
        }
        x = v + static_cast<int64_t>(sz);
    }
    return a;
}

PALACE_BAM_FN bool is_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }      // isspace of the C locale
PALACE_BAM_FN bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// parseSAItem's cut of one item [b, e) (generate_graph.cpp:185-206): six comma fields in getline's sense -- a field exists iff at
// least one byte, possibly just its delimiter, is left -- trimmed at both ends; an empty name or position fails the item
struct SaFields { int64_t b[6], e[6]; };
PALACE_BAM_FN bool sa_fields(const uint8_t *d, int64_t b, int64_t e, SaFields *f)
{
    int64_t p = b;
    PALACE_BAM_UNROLL
    for (int k = 0; k < 6; k++) {
        if (p >= e) return false;                                            // nothing left: getline fails
        int64_t q = p;
        while (q < e && d[q] != ',') q++;
        f->b[k] = p;
        f->e[k] = q;
        p = q < e ? q + 1 : e;
    }
    PALACE_BAM_UNROLL
    for (int k = 0; k < 6; k++) {
        while (f->b[k] < f->e[k] && is_space(d[f->b[k]])) f->b[k]++;
        while (f->e[k] > f->b[k] && is_space(d[f->e[k] - 1])) f->e[k]--;
    }
    return f->b[0] != f->e[0] && f->b[1] != f->e[1];
}

// glibc's atoi on [b, e): (int) strtol -- optional sign, digits up to the first non-digit, 0 without digits; beyond the range of
// long the value saturates, and the conversion to int keeps its low 32 bits.  (The fields are trimmed: no leading blanks are left.)
PALACE_BAM_FN int32_t atoi_field(const uint8_t *d, int64_t b, int64_t e)
{
    bool neg = false, over = false;
    if (b < e && (d[b] == '-' || d[b] == '+')) { neg = d[b] == '-'; b++; }
    const uint64_t limit = neg ? 0x8000000000000000ull : 0x7fffffffffffffffull;
    uint64_t v = 0;
    for (; b < e && is_digit(d[b]); b++) {
        const uint64_t digit = d[b] - '0';
        if (v > (limit - digit) / 10) over = true;
        else v = v * 10 + digit;
    }
    if (over) v = limit;
    return static_cast<int32_t>(static_cast<uint32_t>(neg ? 0 - v : v));
}

// an SA item's CIGAR text [b, e) through OpScan: any non-digit byte ends an op; empty text leaves the interval [0,0] (:332), clip_s = -1
PALACE_BAM_FN void clip_from_text(const uint8_t *d, int64_t b, int64_t e, palace_sa_item *out)
{
    if (b == e) { out->clip_s2 = -1; out->clip_e2 = 0; out->len2 = 0; return; }
    OpScan sc;
    uint32_t acc = 0;
    for (; b < e; b++) {
        const uint8_t ch = d[b];
        if (is_digit(ch)) acc = acc * 10 + (ch - '0');
        else { sc.add(static_cast<int32_t>(acc), ch == 'S', ch == 'M' || ch == 'I' || ch == 'S' || ch == '=' || ch == 'X'); acc = 0; }
    }
    out->clip_s2 = sc.clip_s(); out->clip_e2 = sc.clip_e(); out->len2 = static_cast<int32_t>(sc.len);
}

// f(fields) for every item of the SA text [p, se) that parses, in list order: split at ';' (:719-720), empty items skipped
template <class F>
PALACE_BAM_FN void sa_text_items(const uint8_t *d, int64_t p, int64_t se, F f)
{
    while (p < se) {
        int64_t ie = p;
        while (ie < se && d[ie] != ';') ie++;
        SaFields fl;
        if (ie > p && sa_fields(d, p, ie, &fl)) f(fl);
        p = ie < se ? ie + 1 : se;
    }
}

// ... of the record's SA list: the first SA:Z field of a record with 0 <= tid < n_ref (:687)
template <class F>
PALACE_BAM_FN void record_sa_items(const uint8_t *d, int64_t s, int32_t n_ref, F f)
{
    const int32_t tid = static_cast<int32_t>(ld32(d, s));
    if (tid < 0 || tid >= n_ref) return;
    const int64_t end = s + static_cast<int64_t>(ld32(d, s - 4));
    const int64_t l_name = d[s + 8], n_cig = ld16(d, s + 12), l_seq = ld32(d, s + 16);
    const RecAux a = record_aux(d, s + 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq, end);
    if (a.sa >= 0) sa_text_items(d, a.sa, a.sa + a.sa_len, f);
}

// The item of one cut.  The contig-name look-up is the caller's: is_own(name, n) = the name is that of the record's own contig
// (r1 == r2 -> skip, :731), tid_of(name, n) = its tid, -1 for a name the header does not have (-> skip, :733-734)
template <class Own, class TidOf>
PALACE_BAM_FN palace_sa_item sa_item(const uint8_t *d, const SaFields &f, Own is_own, TidOf tid_of)
{
    palace_sa_item it;
    const uint8_t *name = d + f.b[0];
    const int64_t name_n = f.e[0] - f.b[0];
    it.tid2 = is_own(name, name_n) ? -1 : tid_of(name, name_n);
    it.pos2 = atoi_field(d, f.b[1], f.e[1]);
    it.rev2 = (f.e[2] - f.b[2] == 1 && d[f.b[2]] == '-') ? 1 : 0;
    clip_from_text(d, f.b[3], f.e[3], &it);
    it.mapq2 = atoi_field(d, f.b[4], f.e[4]);
    it.nm2 = atoi_field(d, f.b[5], f.e[5]);
    return it;
}

}  // namespace palace
