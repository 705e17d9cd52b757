// corrected_dup_selftest < case: the host half of corrected_dup (corrected_dup_rules.hpp: the token grammar, the surgery of one path,
// the double arithmetic, the order of the output) on its own, with the device's four answers worked out here by brute force from
// their statements in include/palace_hip.h.  No device call is made and libpalace_hip.so is not linked; the _asan twin runs the
// same under ASan + UBSan (tests/test_host_corrected_dup_selftest.py feeds both every case of tests/golden/corrected_dup_cases.npz).
// The case on stdin, words separated by white space:
//   fai N, then N rows `name length sum covered` (covered 0: no depth);  cycles N, then N rows `k token*k`;  finals N, likewise;
//   cuts N, then N rows `k token*k m token*m` (key, value);  min_len V.  A token is row << 1 | strand.
// stdout: the lines of final.txt, a line `--`, the warning lines.  `corrected_dup_selftest words` instead reads one word a line and
// prints its fault, or `ok`.
#include <iostream>
#include <set>
#include <string>
#include <vector>

#include "corrected_dup_rules.hpp"

namespace cdup = palace_host::cdup;
using cdup::Path;

struct Brute {
    const std::vector<int64_t> &fai_len;

    std::vector<int32_t> borders(const std::vector<Path> &paths)
    {
        std::vector<int32_t> out;
        for (const Path &p : paths) {
            int32_t best = 0;
            for (size_t i = 1; i <= p.size() / 2; i++)
                if (std::equal(p.begin(), p.begin() + static_cast<std::ptrdiff_t>(i), p.end() - static_cast<std::ptrdiff_t>(i))) best = static_cast<int32_t>(i);
            out.push_back(best);
        }
        return out;
    }
    void tandems(const std::vector<Path> &paths, std::vector<cdup::Candidate> *cand, std::vector<int64_t> *cand_off)
    {
        cand->clear();
        cand_off->assign(1, 0);
        for (const Path &p : paths) {
            const size_t n = p.size();
            for (size_t r = 1; r <= n / 2; r++)
                for (size_t s = 0; s + 2 * r <= n; s++) {
                    size_t q = s;
                    while (q + r < n && p[q] == p[q + r]) q++;
                    const size_t c = 1 + (q - s) / r;
                    if (c >= 2) cand->push_back(cdup::Candidate{static_cast<int32_t>(r), static_cast<int32_t>(s), static_cast<int32_t>(c)});
                }
            cand_off->push_back(static_cast<int64_t>(cand->size()));
        }
    }
    std::vector<uint8_t> relation(const std::vector<Path> &paths)
    {
        const size_t n = paths.size();
        std::vector<std::set<int64_t>> d(n);
        std::vector<int64_t> sum(n, 0);
        for (size_t k = 0; k < n; k++) {
            for (const int32_t t : paths[k]) d[k].insert(fai_len[static_cast<size_t>(cdup::base_of(t))]);
            for (const int64_t v : d[k]) sum[k] += v;
        }
        std::vector<uint8_t> rel((n * n + 3) / 4, 0);
        for (size_t i = 0; i < n; i++)
            for (size_t j = i + 1; j < n; j++) {
                int64_t inter = 0;
                for (const int64_t v : d[i]) inter += d[j].count(v) ? v : 0;
                const bool similar = sum[i] == 0 || sum[j] == 0 || static_cast<double>(inter) / static_cast<double>(sum[i]) >= 0.9 ||
                                     static_cast<double>(inter) / static_cast<double>(sum[j]) >= 0.9;
                const size_t k = i * n + j;
                if (similar) rel[k >> 2] |= static_cast<uint8_t>((sum[i] > sum[j] ? cdup::kRelJLoses : cdup::kRelILoses) << (2 * (k & 3)));
            }
        return rel;
    }
    std::vector<uint8_t> base_set_in(const std::vector<Path> &paths, size_t n_cycles)
    {
        std::vector<std::set<int32_t>> b(paths.size());
        for (size_t k = 0; k < paths.size(); k++)
            for (const int32_t t : paths[k]) b[k].insert(cdup::base_of(t));
        std::vector<uint8_t> in(paths.size(), 0);
        for (size_t k = n_cycles; k < paths.size(); k++)
            for (size_t c = 0; c < n_cycles && !in[k]; c++) in[k] = b[k] == b[c];
        return in;
    }
};

static bool expect(const char *word)
{
    std::string w;
    return (std::cin >> w) && w == word;
}

static bool read_path(Path *p)
{
    size_t k = 0;
    if (!(std::cin >> k)) return false;
    p->assign(k, 0);
    for (int32_t &t : *p)
        if (!(std::cin >> t)) return false;
    return true;
}

static bool read_paths(const char *word, std::vector<Path> *out)
{
    size_t n = 0;
    if (!expect(word) || !(std::cin >> n)) return false;
    out->assign(n, Path());
    for (Path &p : *out)
        if (!read_path(&p)) return false;
    return true;
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::string(argv[1]) == "words") {
        std::string w;
        while (std::getline(std::cin, w)) {
            const char *why = cdup::token_fault(w);
            std::cout << (*why ? why : "ok") << "\n";
        }
        return 0;
    }
    size_t n_fai = 0;
    if (!expect("fai") || !(std::cin >> n_fai)) return 2;
    std::vector<std::string> name(n_fai);
    std::vector<int64_t> fai_len(n_fai);
    std::vector<cdup::Depth> depth(n_fai);
    std::vector<cdup::NameInfo> info(n_fai);
    for (size_t k = 0; k < n_fai; k++) {
        if (!(std::cin >> name[k] >> fai_len[k] >> depth[k].sum >> depth[k].covered)) return 2;
        if (!cdup::name_info(name[k], &info[k])) { std::cout << "name " << k << " begins with EDGE and has no length\n"; return 1; }
    }
    std::vector<Path> cycles, finals;
    if (!read_paths("cycles", &cycles) || !read_paths("finals", &finals)) return 2;
    size_t n_cuts = 0;
    if (!expect("cuts") || !(std::cin >> n_cuts)) return 2;
    std::vector<std::pair<Path, Path>> cuts(n_cuts);
    for (auto &c : cuts)
        if (!read_path(&c.first) || !read_path(&c.second)) return 2;
    int64_t min_len = 0;
    if (!expect("min_len") || !(std::cin >> min_len)) return 2;
    for (const std::vector<Path> *set : {&cycles, &finals})
        for (const Path &p : *set)
            for (const int32_t t : p)
                if (t < 0 || static_cast<size_t>(t >> 1) >= n_fai) return 2;

    Brute brute{fai_len};
    auto text_of = [&](int32_t t) { return name[static_cast<size_t>(t >> 1)] + ((t & 1) ? '-' : '+'); };
    std::string out, warnings;
    for (const Path &p : cdup::decide(brute, cycles, finals, cuts, depth, fai_len)) {
        const Path q = cdup::quota(p, info, [&](int32_t t) {
            warnings += "Warning: Could not parse node: " + text_of(t) + ". Error: could not convert string to float: '" + info[static_cast<size_t>(t >> 1)].cov_text + "'\n";
        });
        if (cdup::written_length(q, info) <= min_len) continue;
        for (size_t k = 0; k < q.size(); k++) { if (k) out += '\t'; out += text_of(q[k]); }
        out += '\n';
    }
    std::cout << out << "--\n" << warnings;
    return 0;
}
