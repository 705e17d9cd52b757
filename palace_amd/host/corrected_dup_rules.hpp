// corrected_dup on the host (the rules: DESIGN.md 8): the grammar of a token, the list surgery of ONE path and the double arithmetic
// -- what is linear in a path and what needs a libm or a strtod.  Everything that is quadratic or worse, or touches the BAM, is the
// device's (csrc/path_dedup.hip) and comes in here as numbers: a line's border, its tandem candidates, the paths' relation, the
// base-set verdicts.  A token is base << 1 | strand (strand 1: '-'), a base the row of its name in the `.fai`.  Needs the standard
// library only, so corrected_dup_selftest drives it without a device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace palace_host {
namespace cdup {

using Path = std::vector<int32_t>;
struct Candidate { int32_t r, s, c; };
struct Depth { uint64_t sum = 0, covered = 0; };                  // covered == 0: the contig has no depth
constexpr int32_t kRelNone = 0, kRelJLoses = 1, kRelILoses = 2;  // PALACE_PATHS_REL_*

inline int32_t base_of(int32_t tok) { return tok >> 1; }

// ---- the grammar ----------------------------------------------------------------------------------------------------------------------

// EDGE_<digits>_length_<digits>_cov_<[0-9.]+> from text[at] to the end of the name; id / cov: the two fields
inline bool edge_name_at(std::string_view name, size_t at, std::string_view *id = nullptr, std::string_view *cov = nullptr)
{
    auto word = [&](std::string_view w) { if (name.compare(at, w.size(), w) != 0) return false; at += w.size(); return true; };
    auto run = [&](bool dots, std::string_view *out) {
        const size_t from = at;
        while (at < name.size() && ((name[at] >= '0' && name[at] <= '9') || (dots && name[at] == '.'))) at++;
        if (out) *out = name.substr(from, at - from);
        return at > from;
    };
    return word("EDGE_") && run(false, id) && word("_length_") && run(false, nullptr) && word("_cov_") && run(true, cov) && at == name.size();
}

// why a word is no token ("" when it is one): it ends in its strand, holds no other '+', '-' or ':', and the EDGE pattern matches
// all of it or no part of it
inline const char *token_fault(std::string_view w)
{
    if (w.empty() || (w.back() != '+' && w.back() != '-')) return "does not end in '+' or '-'";
    const std::string_view name = w.substr(0, w.size() - 1);
    if (name.find_first_of("+-:") != std::string_view::npos) return "holds a '+', '-' or ':' inside";
    for (size_t at = name.find("EDGE_", 1); at != std::string_view::npos; at = name.find("EDGE_", at + 1))
        if (edge_name_at(name, at)) return "matches the EDGE pattern in part only";
    return "";
}

// field 3 of the '_'-split token, for a token that begins with EDGE: false when it is no decimal number below 2^62
inline bool edge_field3(std::string_view name, int64_t *out)
{
    size_t at = 0;
    for (int k = 0; k < 3; k++) {
        at = name.find('_', at);
        if (at == std::string_view::npos) return false;
        at++;
    }
    const size_t end = std::min(name.find('_', at), name.size());
    if (end == at || end == name.size()) return false;                     // (the last field carries the strand: no number)
    int64_t v = 0;
    for (size_t k = at; k < end; k++) {
        if (name[k] < '0' || name[k] > '9' || v > (1ll << 58)) return false;
        v = v * 10 + (name[k] - '0');
    }
    *out = v;
    return true;
}

// what the quota rule and the length filter need of a name, worked out once per `.fai` row
struct NameInfo {
    bool edge = false;          // the whole token matches the EDGE pattern
    bool cov_ok = false;        // ... and Python's float() takes its cov text
    double cov = 0;
    std::string id, cov_text;
    bool begins_edge = false;   // the name begins with "EDGE": field 3 counts for the written length
    int64_t field3 = 0;
};

inline bool name_info(std::string_view name, NameInfo *info)
{
    std::string_view id, cov;
    *info = NameInfo{};
    if (edge_name_at(name, 0, &id, &cov)) {
        info->edge = true;
        info->id = std::string(id);
        info->cov_text = std::string(cov);
        const size_t dots = static_cast<size_t>(std::count(cov.begin(), cov.end(), '.'));
        info->cov_ok = dots <= 1 && cov.size() > dots;                       // digits with at most one point, one digit at least
        if (info->cov_ok) info->cov = std::strtod(info->cov_text.c_str(), nullptr);
    }
    info->begins_edge = name.compare(0, 4, "EDGE") == 0;
    return !info->begins_edge || edge_field3(name, &info->field3);
}

// ---- one cycle line ---------------------------------------------------------------------------------------------------------------------

// the distinct pieces, in first-seen order with their counts, of `line` cut in front of every token cut() holds for
template <class Cut>
std::vector<std::pair<Path, int64_t>> pieces_before(const Path &line, Cut cut)
{
    std::vector<size_t> at;
    for (size_t k = 0; k < line.size(); k++)
        if (cut(line[k])) at.push_back(k);
    at.push_back(line.size());
    std::vector<std::pair<Path, int64_t>> out;
    for (size_t k = 0; k + 1 < at.size(); k++) {
        Path piece(line.begin() + static_cast<std::ptrdiff_t>(at[k]), line.begin() + static_cast<std::ptrdiff_t>(at[k + 1]));
        auto it = std::find_if(out.begin(), out.end(), [&](const std::pair<Path, int64_t> &p) { return p.first == piece; });
        if (it == out.end()) out.emplace_back(std::move(piece), 1); else it->second++;
    }
    return out;
}

// rule 1: the rotation by the line's border, or the pieces around the most frequent base
inline Path reformat(const Path &s, int32_t border)
{
    const size_t n = s.size();
    Path out;
    if (border > 0) {
        out.assign(s.end() - border, s.end());
        out.insert(out.end(), s.begin(), s.end() - border);
        return out;
    }
    std::unordered_map<int32_t, int64_t> count;
    for (const int32_t t : s) count[base_of(t)]++;
    int32_t top = -1;
    size_t first = 0;
    for (size_t k = 0; k < n; k++)                                           // (the first met of the most frequent)
        if (top < 0 || count[base_of(s[k])] > count[top]) { top = base_of(s[k]); first = k; }
    Path rotated(s.begin() + static_cast<std::ptrdiff_t>(first), s.end());
    rotated.insert(rotated.end(), s.begin(), s.begin() + static_cast<std::ptrdiff_t>(first));
    for (const auto &p : pieces_before(rotated, [&](int32_t t) { return base_of(t) == top; }))
        for (int64_t c = 0; c < p.second; c++) out.insert(out.end(), p.first.begin(), p.first.end());
    return out;
}

inline bool is_sublist(const Path &a, const Path &b) { return std::search(b.begin(), b.end(), a.begin(), a.end()) != b.end(); }

// rule 2: the accepted units among the device's candidates, in discovery order
inline std::vector<Path> accept_units(const Path &line, const Candidate *cand, size_t n_cand)
{
    std::vector<Path> units;
    for (size_t k = 0; k < n_cand; k++) {
        const Path unit(line.begin() + cand[k].s, line.begin() + cand[k].s + cand[k].r);
        bool known = false;
        for (const Path &u : units) {
            Path uu(u);
            uu.insert(uu.end(), u.begin(), u.end());
            if (is_sublist(u, unit) || is_sublist(unit, uu)) { known = true; break; }
        }
        if (!known) units.push_back(unit);
    }
    return units;
}

// Python's round() of a double: to nearest, ties to even (the default rounding mode)
inline int64_t py_round(double x)
{
    const double r = std::nearbyint(x);
    return r >= 9e18 ? INT64_MAX : r <= -9e18 ? INT64_MIN : static_cast<int64_t>(r);
}

// Python's list[a:b] for a list of n entries (negative: from the end)
inline std::pair<size_t, size_t> py_slice(int64_t a, int64_t b, size_t n)
{
    const int64_t len = static_cast<int64_t>(n);
    auto clamp = [&](int64_t v) { if (v < 0) v += len; return static_cast<size_t>(std::min(std::max<int64_t>(v, 0), len)); };
    const size_t lo = clamp(a), hi = clamp(b);
    return {lo, std::max(lo, hi)};
}

// rules 3 and 4: copies by depth, the units pushed back, the cut at the first token.  depth, fai_len: per base
inline Path correct_line(const Path &reformatted, const std::vector<Path> &units, const std::vector<Depth> &depth, const std::vector<int64_t> &fai_len)
{
    Path line = reformatted;
    Path distinct = line;
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    uint64_t total_sum = 0, total_cov = 0;
    std::unordered_map<int32_t, double> mean;
    for (const int32_t t : distinct) {                                       // (a base on both strands counts twice)
        const Depth &d = depth[static_cast<size_t>(base_of(t))];
        if (!d.covered) continue;
        mean[base_of(t)] = static_cast<double>(d.sum) / static_cast<double>(d.covered);
        total_sum += d.sum;
        total_cov += d.covered;
    }
    const double total_mean = total_cov ? static_cast<double>(total_sum) / static_cast<double>(total_cov) : 0.0;
    std::unordered_map<int32_t, int64_t> copy;
    for (const auto &m : mean) copy[m.first] = total_mean > 0 ? py_round(m.second / total_mean) : 1;
    auto copy_of = [&](int32_t base, int64_t absent) { const auto it = copy.find(base); return it == copy.end() ? absent : it->second; };
    auto count_base = [&](const Path &p, int32_t base) { return static_cast<int64_t>(std::count_if(p.begin(), p.end(), [&](int32_t t) { return base_of(t) == base; })); };
    const int64_t first_copy = copy_of(base_of(reformatted[0]), 0);
    for (const Path &unit : units) {
        int64_t low = 10000;
        int32_t low_base = -1;
        for (const int32_t t : unit) {
            const int64_t c = copy_of(base_of(t), 1);
            if (c < low) { low = c; low_base = base_of(t); }
        }
        const int64_t n_copy = std::max<int64_t>(1, low - (low_base < 0 ? 0 : count_base(reformatted, low_base)));
        Path uu(unit);
        uu.insert(uu.end(), unit.begin(), unit.end());
        int64_t a = -1, b = -1;                                              // the script's search: (-1, -1 + len) when unit unit is gone
        if (!line.empty()) {
            int64_t last = -1;
            for (size_t k = 0; k + uu.size() <= line.size(); k++)
                if (std::equal(uu.begin(), uu.end(), line.begin() + static_cast<std::ptrdiff_t>(k))) { if (a < 0) a = static_cast<int64_t>(k); last = static_cast<int64_t>(k); }
            b = last + static_cast<int64_t>(uu.size());
        }
        const auto head = py_slice(0, a, line.size()), tail = py_slice(b, static_cast<int64_t>(line.size()), line.size());
        Path next(line.begin() + static_cast<std::ptrdiff_t>(head.first), line.begin() + static_cast<std::ptrdiff_t>(head.second));
        for (int64_t c = 0; c < n_copy; c++) next.insert(next.end(), unit.begin(), unit.end());
        next.insert(next.end(), line.begin() + static_cast<std::ptrdiff_t>(tail.first), line.begin() + static_cast<std::ptrdiff_t>(tail.second));
        line.swap(next);
    }
    const int32_t head = line[0];
    const int64_t seen = count_base(line, base_of(head));
    if (std::llabs(seen - first_copy) <= 1) return line;
    Path best;
    int64_t best_len = 0;
    for (const auto &p : pieces_before(line, [&](int32_t t) { return t == head; })) {
        int64_t len = 0;
        for (const int32_t t : p.first) len += fai_len[static_cast<size_t>(base_of(t))];
        if (len > best_len) { best = p.first; best_len = len; }
    }
    return best;
}

// the greedy pass over the relation's codes, rel(i, j) for i < j -> the kept indices
template <class Rel>
std::vector<size_t> greedy_keep(size_t n, Rel rel)
{
    std::vector<uint8_t> kept(n, 1);
    for (size_t i = 0; i < n; i++) {
        if (!kept[i]) continue;
        for (size_t j = i + 1; j < n; j++) {
            if (!kept[j]) continue;
            const int32_t code = rel(i, j);
            if (code == kRelJLoses) kept[j] = 0;
            else if (code == kRelILoses) { kept[i] = 0; break; }
        }
    }
    std::vector<size_t> out;
    for (size_t i = 0; i < n; i++)
        if (kept[i]) out.push_back(i);
    return out;
}

// ---- the paths of the output ------------------------------------------------------------------------------------------------------------

// the kept indices of `paths` under the greedy pass over their relation
template <class Device>
std::vector<size_t> keep_dissimilar(Device &device, const std::vector<Path> &paths)
{
    if (paths.empty()) return {};
    const std::vector<uint8_t> rel = device.relation(paths);
    const size_t n = paths.size();
    return greedy_keep(n, [&](size_t i, size_t j) { const size_t k = i * n + j; return (rel[k >> 2] >> (2 * (k & 3))) & 3; });
}

// The surviving paths in output order, before the quota rule.  device answers what is quadratic or worse: borders(paths),
// tandems(paths, &candidates, &their offsets), relation(paths) and base_set_in(paths, n_cycles), as include/palace_hip.h states them.
// cuts: the rows of before_cut as (key, value), in file order.
template <class Device>
std::vector<Path> decide(Device &device, const std::vector<Path> &original, const std::vector<Path> &final_lines, const std::vector<std::pair<Path, Path>> &cuts,
                         const std::vector<Depth> &depth, const std::vector<int64_t> &fai_len)
{
    // the cycles: border, reformat, tandem candidates, copies by depth, the greedy pass
    std::vector<Path> corrected;
    if (!original.empty()) {
        const std::vector<int32_t> border = device.borders(original);
        std::vector<Path> lines;
        for (size_t k = 0; k < original.size(); k++) lines.push_back(reformat(original[k], border[k]));
        std::vector<Candidate> cand;
        std::vector<int64_t> cand_off;
        device.tandems(lines, &cand, &cand_off);
        for (size_t k = 0; k < lines.size(); k++) {
            const std::vector<Path> units = accept_units(lines[k], cand.data() + cand_off[k], static_cast<size_t>(cand_off[k + 1] - cand_off[k]));
            corrected.push_back(correct_line(lines[k], units, depth, fai_len));
        }
    }
    std::vector<Path> kept_cycles;
    for (const size_t k : keep_dissimilar(device, corrected)) kept_cycles.push_back(corrected[k]);

    // before_cut: key -> value, later rows override; value -> key, the later key of equal values wins
    std::vector<std::pair<Path, Path>> entry;
    std::map<Path, size_t> at, back;
    for (const auto &row : cuts) {
        const auto it = at.find(row.first);
        if (it == at.end()) { at[row.first] = entry.size(); entry.push_back(row); } else entry[it->second].second = row.second;
    }
    for (size_t k = 0; k < entry.size(); k++) back[entry[k].second] = k;

    // the final lines: replaced through before_cut, dropped when a cycle line has their set of bases
    std::vector<Path> all(kept_cycles);
    if (!final_lines.empty()) {
        std::vector<Path> both(original);
        for (const Path &p : final_lines) {
            const auto it = at.find(p);
            both.push_back(it == at.end() ? p : entry[it->second].second);
        }
        const std::vector<uint8_t> in = device.base_set_in(both, original.size());
        for (size_t k = original.size(); k < both.size(); k++)
            if (!in[k]) all.push_back(both[k]);
    }
    std::vector<Path> first, second;
    for (const size_t k : keep_dissimilar(device, all)) {
        const Path &p = all[k];
        if (std::find(kept_cycles.begin(), kept_cycles.end(), p) != kept_cycles.end()) { first.push_back(p); continue; }
        const auto it = back.find(p);
        second.push_back(it == back.end() ? p : entry[it->second].first);
    }
    first.insert(first.end(), second.begin(), second.end());
    return first;
}

// ---- the quota rule ---------------------------------------------------------------------------------------------------------------------

inline double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}

// the path after the quota rule; a node whose cov is no number is reported through warn(token)
template <class Warn>
Path quota(const Path &path, const std::vector<NameInfo> &info, Warn warn)
{
    struct Node { int32_t tok; const std::string *id; double cov; };
    std::vector<Node> nodes;
    for (const int32_t t : path) {
        const NameInfo &ni = info[static_cast<size_t>(base_of(t))];
        if (!ni.edge) continue;
        if (!ni.cov_ok) { warn(t); continue; }
        nodes.push_back(Node{t, &ni.id, ni.cov});
    }
    if (nodes.empty()) return path;
    std::unordered_map<std::string, int64_t> seen;
    for (const Node &n : nodes) seen[*n.id]++;
    std::vector<double> single, all;
    for (const Node &n : nodes) {
        all.push_back(n.cov);
        if (seen[*n.id] == 1) single.push_back(n.cov);
    }
    double baseline = median(single.empty() ? all : single);
    if (baseline == 0) baseline = 1.0;
    std::unordered_map<std::string, double> top;
    for (const Node &n : nodes) {
        const auto it = top.find(*n.id);
        if (it == top.end()) top[*n.id] = std::max(0.0, n.cov); else it->second = std::max(it->second, n.cov);
    }
    std::unordered_map<std::string, int64_t> budget;
    for (const auto &t : top) budget[t.first] = t.second > 2.5 * baseline ? 999999 : std::max<int64_t>(1, py_round(t.second / baseline));
    Path out;
    for (const Node &n : nodes) {
        int64_t &left = budget[*n.id];
        if (left <= 0) continue;
        left--;
        if (out.empty() || out.back() != n.tok) out.push_back(n.tok);
    }
    return out.empty() ? path : out;
}

// the written length of a path: field 3 of every name that begins with EDGE
inline int64_t written_length(const Path &path, const std::vector<NameInfo> &info)
{
    int64_t n = 0;
    for (const int32_t t : path) {
        const NameInfo &ni = info[static_cast<size_t>(base_of(t))];
        if (ni.begins_edge) n += ni.field3;
    }
    return n;
}

}  // namespace cdup
}  // namespace palace_host
