// The lines and tokens of make_final_fa's two small inputs, and nothing else -- no device, no file.
// Both files: lines end at LF and are counted from 1, a last line without LF is a line, a CR directly before the LF is dropped;
// every other byte of a line must be TAB, space or 0x21-0x7E.  Fields are separated by runs of TAB and space.
//   graph: a line that begins with "JUNC" and has five fields or more gives the arc f1+f2 -> f3+f4 and its conjugate
//          f3+flip(f4) -> f1+flip(f2); f2 and f4 must be "+" or "-"; every other line gives nothing.
//   paths: a line, stripped, that is empty or holds "all" anywhere gives nothing; any other line is a path, its fields the tokens;
//          a path holds fewer than 2^20 tokens.
// A node (f1+f2, f3+f4) and a token must hold "length_" followed by 1 to 12 digits; the first such place is the length.
// The smallest faulty line of a file is its fault.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <string_view>
#include <vector>

namespace palace_host {

using fsv = std::string_view;

struct FinalFault {
    int64_t line = 0;                            // 1-based; 0: none
    const char *reason = nullptr;
};

constexpr const char *kFinalBadByte = "a byte other than TAB, space and 0x21-0x7E (a CR is allowed directly before the LF)";
constexpr const char *kFinalBadOrientation = "an orientation field of a JUNC line that is neither '+' nor '-'";
constexpr const char *kFinalNoLength = "a node without 'length_' and 1 to 12 digits behind it";
constexpr const char *kFinalTooManyTokens = "a path of 2^20 tokens or more";
constexpr int64_t kFinalMaxTokens = 1ll << 20;

// strings one behind the other
struct FinalStrings {
    std::string bytes;
    std::vector<int64_t> off{0};
    size_t size() const { return off.size() - 1; }
    fsv at(size_t k) const { return fsv(bytes).substr(static_cast<size_t>(off[k]), static_cast<size_t>(off[k + 1] - off[k])); }
    void add(fsv a, fsv b = fsv())
    {
        bytes.append(a);
        bytes.append(b);
        off.push_back(static_cast<int64_t>(bytes.size()));
    }
};

struct FinalGraph {
    FinalStrings nodes;                          // arc k: nodes 2k -> 2k + 1 (a JUNC line gives two arcs: its own, its conjugate)
    std::vector<int64_t> len;                    // per node
    FinalFault fault;
};

struct FinalPaths {
    FinalStrings tokens;
    std::vector<int64_t> len;                    // per token
    std::vector<int64_t> line_tok{0};            // path k holds the tokens line_tok[k] .. line_tok[k + 1]
    std::vector<int64_t> line_no;                // ... and stands on this line (1-based)
    FinalFault fault;
    size_t paths() const { return line_no.size(); }
};

// the digits behind the first "length_" that has digits behind it; -1: none, or more than 12
inline int64_t final_length(fsv s)
{
    for (size_t at = s.find("length_"); at != fsv::npos; at = s.find("length_", at + 1)) {
        size_t d = at + 7, e = d;
        while (e < s.size() && s[e] >= '0' && s[e] <= '9') e++;
        if (e == d) continue;
        if (e - d > 12) return -1;
        int64_t v = 0;
        for (; d < e; d++) v = v * 10 + (s[d] - '0');
        return v;
    }
    return -1;
}

// a token without every trailing '+' and '-'
inline fsv final_base(fsv token)
{
    while (!token.empty() && (token.back() == '+' || token.back() == '-')) token.remove_suffix(1);
    return token;
}

// what is looked up in the assembly for a token: every "ref" removed (left to right, as str.replace), then the last byte as the
// strand -- '-' reversed, anything else forward, written '+' -- and the bytes before it as the name
inline std::string final_query(fsv token)
{
    std::string q;
    for (size_t i = 0; i < token.size();) {
        if (token.compare(i, 3, "ref") == 0) i += 3;
        else q.push_back(token[i++]);
    }
    if (!q.empty() && q.back() != '-') q.back() = '+';
    return q;
}

namespace final_detail {

inline bool blank(char c) { return c == ' ' || c == '\t'; }

// calls f(1-based line number, line) for every line, the CR before an LF dropped; false when f says stop
template <class F>
inline void each_line(const char *p, size_t n, F f)
{
    int64_t no = 0;
    for (size_t a = 0; a < n;) {
        const void *lf = std::memchr(p + a, '\n', n - a);
        const size_t e = lf ? static_cast<size_t>(static_cast<const char *>(lf) - p) : n;
        size_t t = e;
        if (lf && t > a && p[t - 1] == '\r') t--;
        if (!f(++no, fsv(p + a, t - a))) return;
        a = e + 1;
    }
}

inline bool bytes_ok(fsv line)
{
    for (const char c : line) {
        const unsigned char u = static_cast<unsigned char>(c);
        if (u != '\t' && (u < 0x20 || u > 0x7e)) return false;
    }
    return true;
}

inline void fields(fsv line, std::vector<fsv> &out)
{
    out.clear();
    size_t a = 0;
    while (a < line.size()) {
        while (a < line.size() && blank(line[a])) a++;
        size_t b = a;
        while (b < line.size() && !blank(line[b])) b++;
        if (b > a) out.push_back(line.substr(a, b - a));
        a = b;
    }
}

}  // namespace final_detail

inline FinalGraph final_graph(const char *p, size_t n)
{
    FinalGraph g;
    std::vector<fsv> f;
    final_detail::each_line(p, n, [&](int64_t no, fsv line) {
        if (!final_detail::bytes_ok(line)) { g.fault = FinalFault{no, kFinalBadByte}; return false; }
        if (line.substr(0, 4) != "JUNC") return true;
        final_detail::fields(line, f);
        if (f.size() < 5) return true;
        if ((f[2] != "+" && f[2] != "-") || (f[4] != "+" && f[4] != "-")) { g.fault = FinalFault{no, kFinalBadOrientation}; return false; }
        const int64_t l1 = final_length(f[1]), l2 = final_length(f[3]);
        if (l1 < 0 || l2 < 0) { g.fault = FinalFault{no, kFinalNoLength}; return false; }
        g.nodes.add(f[1], f[2]);
        g.nodes.add(f[3], f[4]);
        g.nodes.add(f[3], f[4] == "-" ? "+" : "-");
        g.nodes.add(f[1], f[2] == "-" ? "+" : "-");
        for (const int64_t l : {l1, l2, l2, l1}) g.len.push_back(l);
        return true;
    });
    if (g.fault.line) { g.nodes = FinalStrings(); g.len.clear(); }
    return g;
}

inline FinalPaths final_paths(const char *p, size_t n)
{
    FinalPaths out;
    std::vector<fsv> f;
    final_detail::each_line(p, n, [&](int64_t no, fsv line) {
        if (!final_detail::bytes_ok(line)) { out.fault = FinalFault{no, kFinalBadByte}; return false; }
        if (line.find("all") != fsv::npos) return true;
        final_detail::fields(line, f);
        if (f.empty()) return true;
        if (static_cast<int64_t>(f.size()) >= kFinalMaxTokens) { out.fault = FinalFault{no, kFinalTooManyTokens}; return false; }
        for (const fsv t : f) {
            const int64_t l = final_length(t);
            if (l < 0) { out.fault = FinalFault{no, kFinalNoLength}; return false; }
            out.tokens.add(t);
            out.len.push_back(l);
        }
        out.line_no.push_back(no);
        out.line_tok.push_back(static_cast<int64_t>(out.tokens.size()));
        return true;
    });
    if (out.fault.line) out = FinalPaths{FinalStrings(), {}, {0}, {}, out.fault};
    return out;
}

}  // namespace palace_host
