// The rules of one SAM alignment line as `samview` encodes it into a BAM record, stated once: the cut into fields, the
// numeric fields, the CIGAR text, SEQ's nibbles, QUAL, the tags, and what the record's refID / pos / flag / bin become.  This one
// text is compiled by hipcc for the kernels of sam.hip -- where a wavefront owns a line and its lanes stride the bytes -- and by the
// host compiler for host/sam_line_selftest_main.cpp, where sam_line_size / sam_line_write run the same pieces one after the other.
// Written against the SAM specification (1.4, 4.2); htslib is not on this machine, so these rules are the behaviour (parity UNPINNED).
//
// Every function is a pure function of the text `t` and offsets into it: no allocation, no library call, nothing of HIP.  A line is
// [b, e) without its LF; field k is [c[k], c[k + 1] - 1).  An error is one of the PALACE_SAM_E* codes of include/palace_hip.h; where
// a line has several, the first in the order of sam_line_size's checks is the line's.
#pragma once
#include <cstdint>

#include "bam_record.hpp"

namespace palace {

PALACE_BAM_FN void st8(uint8_t *o, int64_t at, uint32_t v) { o[at] = static_cast<uint8_t>(v); }
PALACE_BAM_FN void st16(uint8_t *o, int64_t at, uint32_t v) { o[at] = static_cast<uint8_t>(v); o[at + 1] = static_cast<uint8_t>(v >> 8); }
PALACE_BAM_FN void st32(uint8_t *o, int64_t at, uint32_t v)
{
    o[at] = static_cast<uint8_t>(v); o[at + 1] = static_cast<uint8_t>(v >> 8); o[at + 2] = static_cast<uint8_t>(v >> 16); o[at + 3] = static_cast<uint8_t>(v >> 24);
}

// Decimal in [b, e): an optional '-' where `sign`, then one or more digits and nothing else.  0 = *v is the value and lies in
// [lo, hi]; 1 = not such a text; 2 = out of range (the value saturates far outside every range asked for).  No hex, no octal, no '+'.
PALACE_BAM_FN int sam_dec(const uint8_t *t, int64_t b, int64_t e, bool sign, int64_t lo, int64_t hi, int64_t *v)
{
    bool neg = false;
    if (sign && b < e && t[b] == '-') { neg = true; b++; }
    if (b >= e) return 1;
    int64_t a = 0;
    for (int64_t p = b; p < e; p++) {
        if (!is_digit(t[p])) return 1;
        if (a < (1ll << 40)) a = a * 10 + (t[p] - '0');
    }
    if (neg) a = -a;
    *v = a;
    return a < lo || a > hi ? 2 : 0;
}

// ---- the cut ------------------------------------------------------------------------------------------------------------------
// c[0 .. 10]: the begin of fields 1 to 11; c[11]: the begin of the first tag, e + 1 without one.  n_fields < 11: the rest is undefined.
struct SamCuts { int64_t c[12]; int64_t n_fields; };
PALACE_BAM_FN SamCuts sam_cuts(const uint8_t *t, int64_t b, int64_t e)
{
    SamCuts s;
    s.c[0] = b;
    s.n_fields = 1;
    for (int64_t p = b; p < e; p++)
        if (t[p] == '\t') {
            if (s.n_fields < 12) s.c[s.n_fields] = p + 1;
            s.n_fields++;
        }
    if (s.n_fields == 11) s.c[11] = e + 1;
    return s;
}

// ---- QNAME, FLAG, RNAME, POS, MAPQ / RNEXT, PNEXT, TLEN ---------------------------------------------------------------------------
// code_a: the first error among the five fields in front of the CIGAR, code_b: among the three behind it.  tid / mtid as looked up
// (-1 for '*'; mtid = -2 for '='), pos1 / pnext1 as written (1-based).  tid_of(p, n): the target's index, -1 for a name the header lacks.
struct SamHead { int32_t code_a, code_b, flag, mapq, tid, mtid, l_name; int64_t pos1, pnext1, tlen; };
template <class TidOf>
PALACE_BAM_FN SamHead sam_head(const uint8_t *t, const int64_t *c, TidOf tid_of)
{
    SamHead h{0, 0, 0, 0, -1, -1, 0, 0, 0, 0};
    int64_t v = 0;
    auto star = [&](int k) { return c[k + 1] - 1 - c[k] == 1 && t[c[k]] == '*'; };
    auto first = [](int32_t *code, int32_t x) { if (!*code) *code = x; };
    const int64_t nl = c[1] - 1 - c[0];
    bool name_ok = nl >= 1 && nl <= 254;
    for (int64_t p = c[0]; name_ok && p < c[1] - 1; p++) name_ok = t[p] >= '!' && t[p] <= '~';
    if (!name_ok) first(&h.code_a, PALACE_SAM_EQNAME);
    h.l_name = static_cast<int32_t>(nl + 1);
    if (sam_dec(t, c[1], c[2] - 1, false, 0, 65535, &v)) first(&h.code_a, PALACE_SAM_EFLAG); else h.flag = static_cast<int32_t>(v);
    if (!star(2)) {
        h.tid = c[3] - 1 > c[2] ? tid_of(t + c[2], c[3] - 1 - c[2]) : -1;
        if (h.tid < 0) first(&h.code_a, PALACE_SAM_ERNAME);
    }
    if (sam_dec(t, c[3], c[4] - 1, false, 0, 0x7fffffffll, &v)) first(&h.code_a, PALACE_SAM_EPOS); else h.pos1 = v;
    if (sam_dec(t, c[4], c[5] - 1, false, 0, 255, &v)) first(&h.code_a, PALACE_SAM_EMAPQ); else h.mapq = static_cast<int32_t>(v);
    if (c[7] - 1 - c[6] == 1 && t[c[6]] == '=') h.mtid = -2;
    else if (!star(6)) {
        h.mtid = c[7] - 1 > c[6] ? tid_of(t + c[6], c[7] - 1 - c[6]) : -1;
        if (h.mtid < 0) first(&h.code_b, PALACE_SAM_ERNEXT);
    }
    if (sam_dec(t, c[7], c[8] - 1, false, 0, 0x7fffffffll, &v)) first(&h.code_b, PALACE_SAM_EPNEXT); else h.pnext1 = v;
    if (sam_dec(t, c[8], c[9] - 1, true, -0x80000000ll, 0x7fffffffll, &v)) first(&h.code_b, PALACE_SAM_ETLEN); else h.tlen = v;
    return h;
}

// ---- CIGAR --------------------------------------------------------------------------------------------------------------------
PALACE_BAM_FN int sam_op_code(uint8_t ch)
{
    switch (ch) {
    case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
    case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
    default: return -1;
    }
}
// the op whose letter stands at i of the CIGAR text that begins at b: its length is the digits in front of the letter; false: there
// is no digit, or the length is 2^28 or more
PALACE_BAM_FN bool sam_cigar_op(const uint8_t *t, int64_t b, int64_t i, uint32_t *len)
{
    int64_t s = i;
    while (s > b && is_digit(t[s - 1])) s--;
    int64_t v = 0;
    return s < i && sam_dec(t, s, i, false, 0, (1 << 28) - 1, &v) == 0 ? (*len = static_cast<uint32_t>(v), true) : false;
}
struct SamCigar { int32_t code; int64_t n_ops, qlen, rlen; };
// one byte's share: f(ordinal-free) -- the caller counts the letters in front.  bad = the byte is no part of a CIGAR
struct SamCigarByte { bool bad, op; uint32_t word; int64_t q, r; };
PALACE_BAM_FN SamCigarByte sam_cigar_byte(const uint8_t *t, int64_t b, int64_t e, int64_t i)
{
    SamCigarByte x{false, false, 0, 0, 0};
    const int op = sam_op_code(t[i]);
    if (op < 0) { x.bad = !is_digit(t[i]) || i == e - 1; return x; }        // (the last byte is a letter)
    uint32_t len = 0;
    if (!sam_cigar_op(t, b, i, &len)) { x.bad = true; return x; }
    x.op = true;
    x.word = len << 4 | static_cast<uint32_t>(op);
    if (op == 0 || op == 1 || op == 4 || op == 7 || op == 8) x.q = len;
    if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) x.r = len;
    return x;
}
PALACE_BAM_FN bool sam_is_star(const uint8_t *t, int64_t b, int64_t e) { return e - b == 1 && t[b] == '*'; }
// the whole field, one byte after the other; ops (may be null) gets the op words at ops + 4 k
PALACE_BAM_FN SamCigar sam_cigar(const uint8_t *t, int64_t b, int64_t e, uint8_t *ops)
{
    SamCigar c{0, 0, 0, 0};
    if (sam_is_star(t, b, e)) return c;
    bool bad = b >= e;
    for (int64_t i = b; i < e; i++) {
        const SamCigarByte x = sam_cigar_byte(t, b, e, i);
        bad |= x.bad;
        if (!x.op) continue;
        if (ops && c.n_ops < 65536) st32(ops, 4 * c.n_ops, x.word);
        c.n_ops++; c.qlen += x.q; c.rlen += x.r;
    }
    if (bad || c.n_ops > 65535) c.code = PALACE_SAM_ECIGAR;
    return c;
}

// ---- SEQ and QUAL ---------------------------------------------------------------------------------------------------------------
PALACE_BAM_FN uint32_t sam_nibble(uint8_t ch)
{
    switch (ch >= 'a' && ch <= 'z' ? ch - 32 : ch) {
    case '=': return 0; case 'A': return 1; case 'C': return 2; case 'M': return 3; case 'G': return 4; case 'R': return 5;
    case 'S': return 6; case 'V': return 7; case 'T': return 8; case 'W': return 9; case 'Y': return 10; case 'H': return 11;
    case 'K': return 12; case 'D': return 13; case 'B': return 14;
    default: return 15;
    }
}
// packed byte j of a SEQ of l_seq bytes at b
PALACE_BAM_FN uint32_t sam_seq_byte(const uint8_t *t, int64_t b, int64_t l_seq, int64_t j)
{
    return sam_nibble(t[b + 2 * j]) << 4 | (2 * j + 1 < l_seq ? sam_nibble(t[b + 2 * j + 1]) : 0u);
}
PALACE_BAM_FN bool sam_qual_ok(uint8_t ch) { return ch >= 33 && ch <= 126; }

// ---- tags -----------------------------------------------------------------------------------------------------------------------
// the type an integer is stored as: the smallest of c, s, i for a negative value, of C, S, I otherwise
PALACE_BAM_FN uint8_t sam_int_type(int64_t v)
{
    if (v < 0) return v >= -128 ? 'c' : v >= -32768 ? 's' : 'i';
    return v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I';
}
PALACE_BAM_FN int sam_type_bytes(uint8_t ty) { return ty == 'c' || ty == 'C' ? 1 : ty == 's' || ty == 'S' ? 2 : 4; }
PALACE_BAM_FN bool sam_is_hex(uint8_t ch) { return is_digit(ch) || (ch >= 'A' && ch <= 'F') || (ch >= 'a' && ch <= 'f'); }

// One tag [b, e).  size: its bytes in the record (name, type, value).  type: the type byte written.  For Z and H the value's bytes
// [b + 5, e) go behind the three head bytes and a NUL behind them: `text` = how many (the caller's lanes copy them).
struct SamTag { int32_t code; uint8_t type; int64_t size, v, text; };
// the elements of a B value, f(k, value) for each in order; returns 0 or the first error
template <class F>
PALACE_BAM_FN int32_t sam_b_items(const uint8_t *t, int64_t b, int64_t e, uint8_t sub, int64_t *count, F f)
{
    int64_t lo, hi;
    switch (sub) {
    case 'c': lo = -128; hi = 127; break;
    case 'C': lo = 0; hi = 255; break;
    case 's': lo = -32768; hi = 32767; break;
    case 'S': lo = 0; hi = 65535; break;
    case 'i': lo = -0x80000000ll; hi = 0x7fffffffll; break;
    default: lo = 0; hi = 0xffffffffll; break;
    }
    *count = 0;
    for (int64_t p = b + 6; p < e;) {                                        // t[p] is the ',' in front of an element
        if (t[p] != ',') return PALACE_SAM_ETAG;
        int64_t q = p + 1;
        while (q < e && t[q] != ',') q++;
        int64_t v = 0;
        const int rc = sam_dec(t, p + 1, q, true, lo, hi, &v);
        if (rc) return rc == 1 ? PALACE_SAM_ETAG : PALACE_SAM_ETAGRANGE;
        f(*count, v);
        (*count)++;
        p = q;
    }
    return 0;
}
PALACE_BAM_FN SamTag sam_tag(const uint8_t *t, int64_t b, int64_t e)
{
    SamTag g{0, 0, 0, 0, 0};
    auto alpha = [](uint8_t ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
    if (e - b < 5 || t[b + 2] != ':' || t[b + 4] != ':' || !alpha(t[b]) || !(alpha(t[b + 1]) || is_digit(t[b + 1]))) { g.code = PALACE_SAM_ETAG; return g; }
    const int64_t vb = b + 5;
    switch (t[b + 3]) {
    case 'A':
        if (e - vb != 1 || t[vb] < '!' || t[vb] > '~') g.code = PALACE_SAM_ETAG;
        g.type = 'A'; g.v = t[vb < e ? vb : b]; g.size = 4;
        break;
    case 'i': {
        const int rc = sam_dec(t, vb, e, true, -0x80000000ll, 0xffffffffll, &g.v);
        if (rc) g.code = rc == 1 ? PALACE_SAM_ETAG : PALACE_SAM_ETAGRANGE;
        g.type = sam_int_type(g.v); g.size = 3 + sam_type_bytes(g.type);
        break;
    }
    case 'Z':
        g.type = 'Z'; g.text = e - vb; g.size = 4 + g.text;
        break;
    case 'H':
        g.type = 'H'; g.text = e - vb; g.size = 4 + g.text;
        if (g.text & 1) g.code = PALACE_SAM_ETAGHEX;
        for (int64_t p = vb; p < e && !g.code; p++) if (!sam_is_hex(t[p])) g.code = PALACE_SAM_ETAGHEX;
        break;
    case 'B': {
        const uint8_t sub = vb < e ? t[vb] : 0;
        g.type = 'B';
        if (sub == 'f') { g.code = PALACE_SAM_ETAGFLOAT; break; }
        if (sub != 'c' && sub != 'C' && sub != 's' && sub != 'S' && sub != 'i' && sub != 'I') { g.code = PALACE_SAM_ETAG; break; }
        g.code = sam_b_items(t, b, e, sub, &g.v, [](int64_t, int64_t) {});
        g.size = 8 + sam_type_bytes(sub) * g.v;
        break;
    }
    case 'f': g.code = PALACE_SAM_ETAGFLOAT; break;
    default: g.code = PALACE_SAM_ETAG;
    }
    return g;
}
// the tag's bytes at o + at, all of them but the text of a Z / H value (o[at + 3 .. at + 3 + text) is the caller's)
PALACE_BAM_FN void sam_tag_write(const uint8_t *t, int64_t b, int64_t e, const SamTag &g, uint8_t *o, int64_t at)
{
    o[at] = t[b]; o[at + 1] = t[b + 1]; o[at + 2] = g.type;
    const auto put = [&](int64_t p, int bytes, int64_t v) { for (int k = 0; k < bytes; k++) o[p + k] = static_cast<uint8_t>(static_cast<uint64_t>(v) >> (8 * k)); };
    switch (g.type) {
    case 'A': o[at + 3] = static_cast<uint8_t>(g.v); break;
    case 'Z': case 'H': o[at + 3 + g.text] = 0; break;
    case 'B': {
        const uint8_t sub = t[b + 5];
        const int es = sam_type_bytes(sub);
        int64_t n = 0;
        o[at + 3] = sub;
        st32(o, at + 4, static_cast<uint32_t>(g.v));
        sam_b_items(t, b, e, sub, &n, [&](int64_t k, int64_t v) { put(at + 8 + es * k, es, v); });
        break;
    }
    default: put(at + 3, sam_type_bytes(g.type), g.v);
    }
}

// ---- the record -------------------------------------------------------------------------------------------------------------------
// What the fixed part holds once head, CIGAR and SEQ are known: an RNAME with POS 0 is no place (refID -1, pos -1, the flag as it
// is); no ops on a record whose flag 0x4 is clear sets it; '=' is the refID as encoded; bin = reg2bin over the reference bases, one
// base for flag 0x4 or none, 4680 for pos -1.
struct SamFixed { int32_t tid, pos, mtid, mpos, flag, bin; };
PALACE_BAM_FN SamFixed sam_fixed(const SamHead &h, const SamCigar &c)
{
    SamFixed f;
    f.tid = h.tid; f.pos = static_cast<int32_t>(h.pos1 - 1);
    if (h.tid >= 0 && h.pos1 == 0) f.tid = -1;
    f.flag = h.flag | (c.n_ops == 0 ? 4 : 0);
    f.mtid = h.mtid == -2 ? f.tid : h.mtid;
    f.mpos = static_cast<int32_t>(h.pnext1 - 1);
    const int64_t len = (f.flag & 4) || c.rlen == 0 ? 1 : c.rlen;
    f.bin = f.pos < 0 ? 4680 : static_cast<int32_t>(reg2bin(f.pos, f.pos + len) & 0xffffu);
    return f;
}
// the 36 bytes from block_size to tlen at o + at (size = the record's bytes with the block_size word)
PALACE_BAM_FN void sam_fixed_write(const SamHead &h, const SamFixed &f, int64_t n_ops, int64_t l_seq, int64_t size, uint8_t *o, int64_t at)
{
    st32(o, at, static_cast<uint32_t>(size - 4));
    st32(o, at + 4, static_cast<uint32_t>(f.tid));
    st32(o, at + 8, static_cast<uint32_t>(f.pos));
    st8(o, at + 12, static_cast<uint32_t>(h.l_name));
    st8(o, at + 13, static_cast<uint32_t>(h.mapq));
    st16(o, at + 14, static_cast<uint32_t>(f.bin));
    st16(o, at + 16, static_cast<uint32_t>(n_ops));
    st16(o, at + 18, static_cast<uint32_t>(f.flag));
    st32(o, at + 20, static_cast<uint32_t>(l_seq));
    st32(o, at + 24, static_cast<uint32_t>(f.mtid));
    st32(o, at + 28, static_cast<uint32_t>(f.mpos));
    st32(o, at + 32, static_cast<uint32_t>(h.tlen));
}

// The order of a line's checks, for whoever holds the pieces: too few fields; QNAME, FLAG, RNAME, POS, MAPQ; CIGAR; RNEXT, PNEXT,
// TLEN; an empty SEQ; the CIGAR's query length against SEQ; QUAL; the tags from left to right.
PALACE_BAM_FN int32_t sam_first_code(int32_t head_a, int32_t cigar, int32_t head_b, int32_t seq, int32_t ciglen, int32_t qual, int32_t tags)
{
    return head_a ? head_a : cigar ? cigar : head_b ? head_b : seq ? seq : ciglen ? ciglen : qual ? qual : tags;
}

// The line [b, e), one step after the other (the host's use; the kernels do the same steps with a wavefront's lanes).  size: the
// record's bytes with its block_size word, 0 for a line the mask drops; with `o`, a kept record is written at o + at as well.
struct SamLine { int32_t code; int64_t size; };
template <class TidOf>
PALACE_BAM_FN SamLine sam_line(const uint8_t *t, int64_t b, int64_t e, uint32_t mask, TidOf tid_of, uint8_t *o, int64_t at)
{
    const SamCuts s = sam_cuts(t, b, e);
    if (s.n_fields < 11) return SamLine{PALACE_SAM_EFIELDS, 0};
    const int64_t *c = s.c;
    const SamHead h = sam_head(t, c, tid_of);
    const int64_t ops_at = at + 36 + h.l_name;
    const SamCigar cg = sam_cigar(t, c[5], c[6] - 1, o ? o + ops_at : nullptr);
    const int64_t sb = c[9], se = c[10] - 1, qb = c[10], qe = c[11] - 1;
    const bool seq_star = sam_is_star(t, sb, se), qual_star = sam_is_star(t, qb, qe);
    const int64_t l_seq = seq_star ? 0 : se - sb;
    const int32_t seq_code = se == sb || l_seq > 0x7fffffffll ? PALACE_SAM_ESEQ : 0;
    const int32_t ciglen_code = cg.n_ops > 0 && !seq_star && cg.qlen != l_seq ? PALACE_SAM_ECIGLEN : 0;
    int32_t qual_code = 0;
    if (!qual_star) {
        if (qe - qb != l_seq || qe == qb) qual_code = PALACE_SAM_EQUAL;
        for (int64_t p = qb; p < qe && !qual_code; p++) if (!sam_qual_ok(t[p])) qual_code = PALACE_SAM_EQUAL;
    }
    const int64_t seq_at = ops_at + 4 * cg.n_ops, qual_at = seq_at + (l_seq + 1) / 2, aux_at = qual_at + l_seq;
    int32_t tag_code = 0;
    int64_t aux = 0;
    for (int64_t p = c[11]; p <= e && !tag_code;) {
        int64_t q = p;
        while (q < e && t[q] != '\t') q++;
        const SamTag g = sam_tag(t, p, q);
        tag_code = g.code;
        aux += g.size;
        p = q + 1;
    }
    const int32_t code = sam_first_code(h.code_a, cg.code, h.code_b, seq_code, ciglen_code, qual_code, tag_code);
    if (code) return SamLine{code, 0};
    if (static_cast<uint32_t>(h.flag) & mask) return SamLine{0, 0};
    const int64_t size = 36 + h.l_name + 4 * cg.n_ops + (l_seq + 1) / 2 + l_seq + aux;
    if (!o) return SamLine{0, size};
    sam_fixed_write(h, sam_fixed(h, cg), cg.n_ops, l_seq, size, o, at);
    for (int64_t k = 0; k < h.l_name - 1; k++) o[at + 36 + k] = t[c[0] + k];
    o[at + 36 + h.l_name - 1] = 0;
    for (int64_t j = 0; j < (l_seq + 1) / 2; j++) o[seq_at + j] = static_cast<uint8_t>(sam_seq_byte(t, sb, l_seq, j));
    for (int64_t j = 0; j < l_seq; j++) o[qual_at + j] = qual_star ? 0xff : static_cast<uint8_t>(t[qb + j] - 33);
    int64_t x = aux_at;
    for (int64_t p = c[11]; p <= e;) {
        int64_t q = p;
        while (q < e && t[q] != '\t') q++;
        const SamTag g = sam_tag(t, p, q);
        sam_tag_write(t, p, q, g, o, x);
        for (int64_t k = 0; k < g.text; k++) o[x + 3 + k] = t[p + 5 + k];
        x += g.size;
        p = q + 1;
    }
    return SamLine{0, size};
}

}  // namespace palace
