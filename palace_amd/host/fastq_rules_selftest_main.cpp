// csrc/fastq_rules.hpp on its own, on a CPU (tests/test_host_readqc_rules.py; also built under ASan + UBSan):
//   fastq_rules_selftest <cases>
// one verdict per line of the case file (an empty field is written `.`):
//   G <hex of a text>                                        -> G <records> <smallest faulty line> <code>
//   P <flags: letters of AQL, or -> <seq1> <hex of qual1> <seq2> <hex of qual2>
//                                                            -> P <first accepted candidate or -1> <bases read 1 keeps> <read 2 keeps> <reason>
//   I <flags as above> <seq1> <seq2>                         -> I <first accepted candidate or -1 (-1 under A)> <the insert size's slot>
//   Q <hex of QUAL bytes> <the bases, as many>               -> Q <per byte: slot:value:q20:q30, blank between> (`Q` alone for none)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../csrc/fastq_rules.hpp"

namespace {

std::vector<uint8_t> unhex(const std::string &s)
{
    std::vector<uint8_t> v;
    if (s == ".") return v;
    for (size_t k = 0; k + 1 < s.size(); k += 2) v.push_back(static_cast<uint8_t>(std::strtoul(s.substr(k, 2).c_str(), nullptr, 16)));
    return v;
}
std::vector<uint8_t> bytes_of(const std::string &s) { return s == "." ? std::vector<uint8_t>() : std::vector<uint8_t>(s.begin(), s.end()); }

palace_readqc_params params_of(const std::string &flags)
{
    palace_readqc_params p{15, 40, 5, 15, 0, 0, 0, 30, 5, 20, 50, 0};
    p.no_trim = flags.find('A') != std::string::npos;
    p.no_quality_filter = flags.find('Q') != std::string::npos;
    p.no_length_filter = flags.find('L') != std::string::npos;
    return p;
}

// the first accepted candidate of read 1's bases and read 2's as they stand in the file (-1: none)
int32_t first_accepted(const std::vector<uint8_t> &a, const std::vector<uint8_t> &r2, const palace_readqc_params &p)
{
    std::vector<uint8_t> b(r2.size());
    for (size_t k = 0; k < r2.size(); k++) b[k] = static_cast<uint8_t>(palace::fastq_complement(r2[r2.size() - 1 - k]));
    const int32_t l1 = static_cast<int32_t>(a.size()), l2 = static_cast<int32_t>(b.size());
    const int32_t n_cand = palace::fastq_forward_candidates(l1, p) + palace::fastq_reverse_candidates(l2, p);
    for (int32_t k = 0; k < n_cand; k++)
        if (palace::fastq_accept(a.data(), b.data(), palace::fastq_candidate(k, l1, l2, p), p)) return k;
    return -1;
}

int32_t count_below(const std::vector<uint8_t> &v, int32_t keep, uint32_t below)
{
    int32_t c = 0;
    for (int32_t k = 0; k < keep; k++) c += v[static_cast<size_t>(k)] < below ? 1 : 0;
    return c;
}
int32_t count_n(const std::vector<uint8_t> &v, int32_t keep)
{
    int32_t c = 0;
    for (int32_t k = 0; k < keep; k++) c += v[static_cast<size_t>(k)] == 'N' ? 1 : 0;
    return c;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "Usage: fastq_rules_selftest <cases>\n"); return 2; }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "fastq_rules_selftest: cannot open %s\n", argv[1]); return 2; }
    for (std::string line; std::getline(f, line);) {
        std::istringstream in(line);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "G") {
            std::string hex;
            in >> hex;
            const std::vector<uint8_t> text = unhex(hex);                    // exactly the text's bytes: a read past them is the sanitizer's
            int64_t records, bad_line;
            int32_t code;
            palace::fastq_text_verdict(text.data(), static_cast<int64_t>(text.size()), &records, &bad_line, &code);
            std::printf("G %lld %lld %d\n", static_cast<long long>(records), static_cast<long long>(bad_line), code);
        } else if (kind == "P") {
            std::string flags, s1, q1, s2, q2;
            if (!(in >> flags >> s1 >> q1 >> s2 >> q2)) { std::fprintf(stderr, "fastq_rules_selftest: a P line needs five fields\n"); return 2; }
            const palace_readqc_params p = params_of(flags);
            const std::vector<uint8_t> a = bytes_of(s1), r2 = bytes_of(s2), qa = unhex(q1), qb = unhex(q2);
            if (qa.size() != a.size() || qb.size() != r2.size()) { std::fprintf(stderr, "fastq_rules_selftest: QUAL has not SEQ's length\n"); return 2; }
            const int32_t l1 = static_cast<int32_t>(a.size()), l2 = static_cast<int32_t>(r2.size());
            const int32_t c = first_accepted(a, r2, p);
            const int32_t cut = palace::fastq_trim_to(c, l1, l2, p);
            const int32_t k1 = cut >= 0 && cut < l1 ? cut : l1, k2 = cut >= 0 && cut < l2 ? cut : l2;
            const uint32_t below = 33u + static_cast<uint32_t>(p.qualified_quality);
            const int32_t reason = palace::fastq_pair_reason(palace::fastq_filter(k1, count_below(qa, k1, below), count_n(a, k1), p),
                                                             palace::fastq_filter(k2, count_below(qb, k2, below), count_n(r2, k2), p));
            std::printf("P %d %d %d %d\n", c, k1, k2, reason);
        } else if (kind == "I") {
            std::string flags, s1, s2;
            if (!(in >> flags >> s1 >> s2)) { std::fprintf(stderr, "fastq_rules_selftest: an I line needs three fields\n"); return 2; }
            const palace_readqc_params p = params_of(flags);
            const std::vector<uint8_t> a = bytes_of(s1), r2 = bytes_of(s2);
            const int32_t c = p.no_trim ? -1 : first_accepted(a, r2, p);      // (as the plan: no search under -A)
            std::printf("I %d %d\n", c, palace::fastq_insert_size(c, static_cast<int32_t>(a.size()), static_cast<int32_t>(r2.size()), p));
        } else if (kind == "Q") {
            std::string hex, bases;
            in >> hex >> bases;
            const std::vector<uint8_t> q = unhex(hex), b = bytes_of(bases);
            if (q.size() != b.size()) { std::fprintf(stderr, "fastq_rules_selftest: a Q line needs as many bases as QUAL bytes\n"); return 2; }
            std::printf("Q");
            for (size_t k = 0; k < q.size(); k++)
                std::printf(" %d:%u:%d:%d", palace::fastq_base_slot(b[k]), palace::fastq_qual_value(q[k]), palace::fastq_is_q20(q[k]) ? 1 : 0,
                            palace::fastq_is_q30(q[k]) ? 1 : 0);
            std::printf("\n");
        } else { std::fprintf(stderr, "fastq_rules_selftest: unknown case kind %s\n", kind.c_str()); return 2; }
    }
    return 0;
}
