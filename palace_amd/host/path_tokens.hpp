// The lines and tokens of a paths file as make_fa_from_path reads them, and nothing else: lines end at LF and are
// counted from 0, skipped ones included; a line that begins with "iter" or "self", or is empty once the white space at its ends
// (space, TAB, CR, LF, VT, FF) is gone, gives no record; any other line, stripped, is split at EVERY TAB (two TABs in a row
// give an empty token).  A token is kept twice: as split (the header of the modes other than 0 joins those) and cleaned --
// every space removed, then stripped -- which is what is looked up.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace palace_host {

struct PathTokens {
    std::vector<int64_t> line_index;             // per line that gives a record: its 0-based index in the file
    std::vector<int64_t> line_tok{0};            // ... its tokens are line_tok[k] .. line_tok[k + 1]
    std::string raw, clean;                      // the tokens' bytes, one behind the other
    std::vector<int64_t> raw_off{0}, clean_off{0};
    size_t lines() const { return line_index.size(); }
    size_t tokens() const { return raw_off.size() - 1; }
};

inline bool path_space(char c) { return c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f'; }

inline PathTokens split_paths(const char *p, size_t n)
{
    PathTokens out;
    int64_t index = 0;
    for (size_t a = 0; a < n; index++) {
        const void *lf = std::memchr(p + a, '\n', n - a);
        const size_t e = lf ? static_cast<size_t>(static_cast<const char *>(lf) - p) : n;
        size_t s = a, t = e;
        a = e + 1;
        if (t - s >= 4 && (std::memcmp(p + s, "iter", 4) == 0 || std::memcmp(p + s, "self", 4) == 0)) continue;
        while (s < t && path_space(p[s])) s++;
        while (t > s && path_space(p[t - 1])) t--;
        if (s == t) continue;
        out.line_index.push_back(index);
        for (size_t b = s;; ) {
            const void *tab = std::memchr(p + b, '\t', t - b);
            const size_t c = tab ? static_cast<size_t>(static_cast<const char *>(tab) - p) : t;
            out.raw.append(p + b, c - b);
            out.raw_off.push_back(static_cast<int64_t>(out.raw.size()));
            const size_t before = out.clean.size();
            for (size_t i = b; i < c; i++)
                if (p[i] != ' ') out.clean.push_back(p[i]);
            size_t lo = before, hi = out.clean.size();
            while (lo < hi && path_space(out.clean[lo])) lo++;
            while (hi > lo && path_space(out.clean[hi - 1])) hi--;
            out.clean.erase(hi);
            out.clean.erase(before, lo - before);
            out.clean_off.push_back(static_cast<int64_t>(out.clean.size()));
            if (!tab) break;
            b = c + 1;
        }
        out.line_tok.push_back(static_cast<int64_t>(out.tokens()));
    }
    return out;
}

}  // namespace palace_host
