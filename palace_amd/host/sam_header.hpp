// The header of a SAM text as `samview` takes it, on the host: the '@' lines in front of the first alignment line are
// the BAM header's text, verbatim (no @PG line is added); the targets are the @SQ lines in order, each with an SN and an LN in
// 1 .. 2^31 - 1, no SN twice.  No @SQ line at all is a header of no targets.  Nothing of HIP: sam_line_selftest uses it too.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "../../include/palace_hip.h"

namespace palace_host {

struct SamHeader {
    size_t text_bytes = 0;                 // the header is the text's first text_bytes bytes
    int64_t n_lines = 0;                   // ... and its first n_lines lines
    std::vector<std::string> name;
    std::vector<int32_t> len;
    int code = 0;                          // PALACE_SAM_EHDSQ / _EHDDUP at line `line` (1-based), 0: none
    int64_t line = 0;
};

inline SamHeader parse_sam_header(const uint8_t *t, size_t n)
{
    SamHeader h;
    std::unordered_set<std::string> seen;
    size_t b = 0;
    while (b < n && t[b] == '@') {
        const void *lf = std::memchr(t + b, '\n', n - b);
        const size_t e = lf ? static_cast<size_t>(static_cast<const uint8_t *>(lf) - t) : n;
        h.n_lines++;
        const void *tab = std::memchr(t + b, '\t', e - b);
        const size_t type_end = tab ? static_cast<size_t>(static_cast<const uint8_t *>(tab) - t) : e;
        if (type_end - b == 3 && std::memcmp(t + b, "@SQ", 3) == 0 && !h.code) {
            std::string sn;
            int64_t ln = 0;
            bool have_sn = false, have_ln = false;
            for (size_t f = type_end; f < e;) {                              // t[f] is the TAB in front of a field
                const void *nt = std::memchr(t + f + 1, '\t', e - f - 1);
                const size_t fe = nt ? static_cast<size_t>(static_cast<const uint8_t *>(nt) - t) : e;
                if (fe - f - 1 >= 3 && !have_sn && std::memcmp(t + f + 1, "SN:", 3) == 0) {
                    have_sn = true;
                    sn.assign(reinterpret_cast<const char *>(t) + f + 4, fe - f - 4);
                } else if (fe - f - 1 >= 3 && !have_ln && std::memcmp(t + f + 1, "LN:", 3) == 0) {
                    have_ln = true;
                    bool ok = fe > f + 4;
                    for (size_t p = f + 4; p < fe && ok; p++) {
                        ok = t[p] >= '0' && t[p] <= '9';
                        if (ln < (1ll << 40)) ln = ln * 10 + (t[p] - '0');
                    }
                    if (!ok) ln = 0;
                }
                f = fe;
            }
            if (!have_sn || sn.empty() || !have_ln || ln < 1 || ln > 0x7fffffffll) { h.code = PALACE_SAM_EHDSQ; h.line = h.n_lines; }
            else if (!seen.insert(sn).second) { h.code = PALACE_SAM_EHDDUP; h.line = h.n_lines; }
            else { h.name.push_back(sn); h.len.push_back(static_cast<int32_t>(ln)); }
        }
        b = lf ? e + 1 : n;
    }
    h.text_bytes = b;
    return h;
}

// the BAM header (SAM specification 4.2): magic, l_text, text, n_ref, and per target l_name, name NUL, l_ref
inline std::vector<uint8_t> bam_header_bytes(const SamHeader &h, const uint8_t *t)
{
    std::vector<uint8_t> out{'B', 'A', 'M', 1};
    auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; k++) out.push_back(static_cast<uint8_t>(v >> (8 * k))); };
    put32(static_cast<uint32_t>(h.text_bytes));
    out.insert(out.end(), t, t + h.text_bytes);
    put32(static_cast<uint32_t>(h.name.size()));
    for (size_t k = 0; k < h.name.size(); k++) {
        put32(static_cast<uint32_t>(h.name[k].size() + 1));
        out.insert(out.end(), h.name[k].begin(), h.name[k].end());
        out.push_back(0);
        put32(static_cast<uint32_t>(h.len[k]));
    }
    return out;
}

inline const char *sam_error_text(int code)
{
    switch (code) {
    case PALACE_SAM_EAT: return "a header line ('@') behind the first alignment line";
    case PALACE_SAM_EEMPTY: return "an empty line";
    case PALACE_SAM_EFIELDS: return "fewer than 11 TAB-separated fields";
    case PALACE_SAM_EQNAME: return "QNAME is not 1 to 254 printable bytes";
    case PALACE_SAM_EFLAG: return "FLAG is not a decimal in 0 .. 65535";
    case PALACE_SAM_ERNAME: return "RNAME is neither '*' nor a target of the header";
    case PALACE_SAM_EPOS: return "POS is not a decimal in 0 .. 2147483647";
    case PALACE_SAM_EMAPQ: return "MAPQ is not a decimal in 0 .. 255";
    case PALACE_SAM_ECIGAR: return "CIGAR is neither '*' nor up to 65535 operations <length below 2^28><one of MIDNSHP=X>";
    case PALACE_SAM_ERNEXT: return "RNEXT is none of '*', '=' and a target of the header";
    case PALACE_SAM_EPNEXT: return "PNEXT is not a decimal in 0 .. 2147483647";
    case PALACE_SAM_ETLEN: return "TLEN is not a decimal within int32";
    case PALACE_SAM_ESEQ: return "SEQ is empty";
    case PALACE_SAM_ECIGLEN: return "the CIGAR's query length is not the length of SEQ";
    case PALACE_SAM_EQUAL: return "QUAL is neither '*' nor as many bytes of '!' .. '~' as SEQ has";
    case PALACE_SAM_ETAG: return "a tag that is not XX:T:value with a type of A, i, Z, H, B and a value of that type";
    case PALACE_SAM_ETAGRANGE: return "an integer of a tag outside the range of its type";
    case PALACE_SAM_ETAGFLOAT: return "a tag of type f (or B:f): float tags are not taken";
    case PALACE_SAM_ETAGHEX: return "an H tag that is not an even count of hex digits";
    case PALACE_SAM_EHDSQ: return "an @SQ line without SN, or without an LN in 1 .. 2147483647";
    case PALACE_SAM_EHDDUP: return "an @SQ line whose SN an earlier one has";
    default: return "unknown error";
    }
}

}  // namespace palace_host
