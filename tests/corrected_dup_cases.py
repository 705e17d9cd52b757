"""corrected_dup: the brute-force form of each contract of csrc/path_dedup.hip, the Python model of the rules -- written
from the rules' statement, not from the reference script's text -- and the seeded case generator behind
tests/golden/corrected_dup_cases.npz (tests/golden/make_corrected_dup_golden.py runs the reference script on these cases).

Paths are lists of hashable tokens here; the kernels see the same paths as integers."""
import re

import numpy as np

# ---- the kernels' contracts, by brute force -----------------------------------------------------------------------------------------


def border(path):
    """the largest i in 1 .. n // 2 with path[:i] == path[n - i:], 0 for none"""
    n, best = len(path), 0
    for i in range(1, n // 2 + 1):
        if list(path[:i]) == list(path[n - i:]):
            best = i
    return best


def run_length(path, r, s):
    """R(r, s): the consecutive q >= s with q + r < n and path[q] == path[q + r]"""
    q = s
    while q + r < len(path) and path[q] == path[q + r]:
        q += 1
    return q - s


def tandem_candidates(path):
    """every (r, s, c) with c = 1 + R(r, s) // r >= 2, r ascending, then s ascending -- one loop per start"""
    n, out = len(path), []
    for r in range(1, n // 2 + 1):
        for s in range(0, n - 2 * r + 1):
            c = 1 + run_length(path, r, s) // r
            if c >= 2:
                out.append((r, s, c))
    return out


def tandem_candidates_np(path):
    """the same for long paths: per period, the next position whose flag is 0 -- a search, no suffix scan"""
    a = np.asarray(path, np.int64)
    n, out = len(a), []
    for r in range(1, n // 2 + 1):
        eq = a[:n - r] == a[r:]
        stops = np.append(np.flatnonzero(~eq), n - r)
        s = np.arange(0, n - 2 * r + 1)
        run = stops[np.searchsorted(stops, s)] - s
        keep = run >= r
        out.append(np.stack([np.full(int(keep.sum()), r), s[keep], 1 + run[keep] // r], axis=1))
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 3), np.int32)


REL_NONE, REL_J_LOSES, REL_I_LOSES = 0, 1, 2


def pair_relation(lens_i, lens_j):
    """the rule's similarity of two paths given as their tokens' lengths: IEEE double divisions, as the rule states them (a path whose
    distinct lengths sum to 0 is similar to every path: 10 * 0 >= 9 * 0, the form the entry point computes)"""
    di, dj = set(int(x) for x in lens_i), set(int(x) for x in lens_j)
    si, sj, inter = sum(di), sum(dj), sum(di & dj)
    if si == 0 or sj == 0 or float(inter) / float(si) >= 0.9 or float(inter) / float(sj) >= 0.9:
        return REL_J_LOSES if si > sj else REL_I_LOSES
    return REL_NONE


def length_relation(paths_lens):
    """the n x n table of pair_relation for i < j, 0 elsewhere"""
    n = len(paths_lens)
    rel = np.zeros((n, n), np.uint8)
    for i in range(n):
        for j in range(i + 1, n):
            rel[i, j] = pair_relation(paths_lens[i], paths_lens[j])
    return rel


def greedy_keep(n, rel):
    """the greedy pass over the relation's codes: ascending kept i, ascending kept j > i, the loser is dropped; once i is dropped the
    pass goes on to the next i.  rel(i, j) -> code.  Returns the kept indices, ascending."""
    kept = [True] * n
    for i in range(n):
        if not kept[i]:
            continue
        for j in range(i + 1, n):
            if not kept[j]:
                continue
            code = rel(i, j)
            if code == REL_J_LOSES:
                kept[j] = False
            elif code == REL_I_LOSES:
                kept[i] = False
                break
    return [i for i in range(n) if kept[i]]


def base_set_in(paths_bases, n_cycles):
    """per path: 1 when it is no cycle and its set of bases is that of one of the first n_cycles paths"""
    cycles = [frozenset(p) for p in paths_bases[:n_cycles]]
    return np.array([int(k >= n_cycles and frozenset(p) in cycles) for k, p in enumerate(paths_bases)], np.uint8)


def flatten(paths, dtype=np.int32):
    """paths -> (values back to back, path_off)"""
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    vals = np.array([v for p in paths for v in p], dtype)
    return vals, off


# ---- the model of the rules -------------------------------------------------------------------------------------------

EDGE_RE = re.compile(r"EDGE_(\d+)_length_(\d+)_cov_([0-9.]+)[+-]")

FEATURES = ("no_cycle_line", "border", "merge_repeat", "two_units", "doubled_gone", "both_strands", "unknown_contig", "no_coverage", "total_mean_0",
            "before_cut_replace", "map_back", "base_set_skip", "ratio_exact", "ratio_just_under", "equal_sums", "hub", "budget_cut", "adjacent_collapse",
            "non_edge_dropped", "at_min_len", "at_min_len_plus_1", "first_token_cut")


class Rejected(Exception):
    """an input outside the grammar: (file, 1-based line, reason)"""


def base_of(tok):
    return tok[:-1]


def py_round(x):
    """Python's round() of a double: to nearest, ties to even"""
    return int(round(float(x)))


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else (xs[n // 2 - 1] + xs[n // 2]) / 2.0


def split_before(tokens, is_cut):
    """cut the list in front of every token that is_cut() holds for (what stands before the first such token is no piece) -> the
    distinct pieces in first-seen order with their counts"""
    at = [k for k, t in enumerate(tokens) if is_cut(t)] + [len(tokens)]
    seen = {}
    for a, b in zip(at, at[1:]):
        piece = tuple(tokens[a:b])
        seen[piece] = seen.get(piece, 0) + 1
    return seen


def reformat(tokens, trace):
    n, L = len(tokens), border(tokens)
    if L:
        trace.add("border")
        return tokens[n - L:] + tokens[:n - L]
    trace.add("merge_repeat")
    bases = [base_of(t) for t in tokens]
    counts = {}
    for b in bases:
        counts[b] = counts.get(b, 0) + 1
    top = max(counts, key=counts.get)                                    # (the first of equal counts: dicts keep insertion order)
    k = bases.index(top)
    rotated = tokens[k:] + tokens[:k]
    out = []
    for piece, count in split_before(rotated, lambda t: base_of(t) == top).items():
        out += list(piece) * count
    return out


def is_sublist(a, b):
    return any(list(b[k:k + len(a)]) == list(a) for k in range(len(b) - len(a) + 1))


def tandem_units(tokens, candidates=None):
    """the accepted units in discovery order; candidates: the (r, s, c) of the line (the kernel's contract), by brute force if absent"""
    units = []
    for r, s, _ in (tandem_candidates(tokens) if candidates is None else candidates):
        unit = tokens[s:s + r]
        if not any(is_sublist(u, unit) or is_sublist(unit, u + u) for u in units):
            units.append(unit)
    return units


def find_first_last(a, b):
    """the script's search of a in b: (first, last + len(a)), (-1, -1 + len(a)) when a does not occur, (-1, -1) when either is empty"""
    if not a or not b:
        return -1, -1
    first = last = -1
    for k in range(len(b) - len(a) + 1):
        if b[k:k + len(a)] == a:
            first = k if first == -1 else first
            last = k
    return first, last + len(a)


def correct_cycle(tokens, fai, depth, trace, units=None):
    """rules 1 to 4 of one cycle line; units: pushed back in this order instead of the order of discovery (tests)"""
    line = reformat(tokens, trace)
    units = tandem_units(line) if units is None else units
    if len(units) >= 2:
        trace.add("two_units")
    total_sum = total_cov = 0
    mean = {}
    for tok in dict.fromkeys(line):                                       # the distinct signed tokens
        b = base_of(tok)
        if b not in depth:
            trace.add("unknown_contig")
        elif depth[b][1] == 0:
            trace.add("no_coverage")
        else:
            if b in mean:
                trace.add("both_strands")
            mean[b] = depth[b][0] / depth[b][1]
            total_sum += depth[b][0]
            total_cov += depth[b][1]
    total_mean = total_sum / total_cov if total_cov else 0
    if mean and total_mean == 0:
        trace.add("total_mean_0")
    copy = {b: (py_round(m / total_mean) if total_mean > 0 else 1) for b, m in mean.items()}
    bases = [base_of(t) for t in line]
    first_copy = copy.get(bases[0], 0)
    for unit in units:
        low, low_base = 10000, ""
        for tok in unit:
            c = copy.get(base_of(tok), 1)
            if c < low:
                low, low_base = c, base_of(tok)
        n_copy = max(1, low - bases.count(low_base))
        a, b = find_first_last(unit + unit, line)
        if a == -1:
            trace.add("doubled_gone")
        line = line[:a] + unit * n_copy + line[b:]
    head = line[0]
    if abs(sum(1 for t in line if base_of(t) == base_of(head)) - first_copy) <= 1:
        return line
    trace.add("first_token_cut")
    best, best_len = [], 0
    for piece in split_before(line, lambda t: t == head):
        n = sum(fai[base_of(t)] for t in piece)
        if n > best_len:
            best, best_len = list(piece), n
    return best


def greedy_paths(paths, fai, trace):
    """the greedy pass over the paths' similarity -> the kept indices"""
    lens = [[fai[base_of(t)] for t in p] for p in paths]

    def rel(i, j):
        di, dj = set(lens[i]), set(lens[j])
        si, sj, inter = sum(di), sum(dj), sum(di & dj)
        for s in (si, sj):
            if 10 * inter == 9 * s:
                trace.add("ratio_exact")
            elif 89 * s <= 100 * inter < 90 * s:
                trace.add("ratio_just_under")
        code = pair_relation(lens[i], lens[j])
        if code and si == sj:
            trace.add("equal_sums")
        return code
    return greedy_keep(len(paths), rel)


def quota(path, trace):
    """-> (the path after the quota rule, the warning lines)"""
    nodes, warnings = [], []
    for tok in path:
        m = EDGE_RE.fullmatch(tok)
        if not m:
            continue
        try:
            nodes.append((tok, m.group(1), float(m.group(3))))
        except ValueError:
            warnings.append(f"Warning: Could not parse node: {tok}. Error: could not convert string to float: '{m.group(3)}'\n")
    if not nodes:
        return list(path), warnings
    if len(nodes) < len(path):
        trace.add("non_edge_dropped")
    ids = [n[1] for n in nodes]
    single = [n[2] for n in nodes if ids.count(n[1]) == 1]
    baseline = median(single if single else [n[2] for n in nodes])
    if baseline == 0:
        baseline = 1.0
    top = {}
    for _, uid, cov in nodes:
        top[uid] = max(top.get(uid, 0.0), cov)
    budget = {}
    for uid, cov in top.items():
        if cov > 2.5 * baseline:
            budget[uid] = 999999
            trace.add("hub")
        else:
            budget[uid] = max(1, py_round(cov / baseline))
    kept = []
    for tok, uid, _ in nodes:
        if budget[uid] > 0:
            budget[uid] -= 1
            kept.append(tok)
        else:
            trace.add("budget_cut")
    out = []
    for tok in kept:
        if not out or out[-1] != tok:
            out.append(tok)
        else:
            trace.add("adjacent_collapse")
    return (out if out else list(path)), warnings


def path_len(path):
    return sum(int(t.split("_")[3]) for t in path if t.startswith("EDGE"))


def check_tokens(tokens, fai, name, line_no):
    for t in tokens:
        if t[-1:] not in ("+", "-") or "+" in t[:-1] or "-" in t[:-1] or ":" in t:
            raise Rejected(name, line_no, f"'{t}' is no token")
        if t[:-1] not in fai:
            raise Rejected(name, line_no, f"'{t[:-1]}' is no sequence of the index")


def parse_inputs(case):
    fai = {}
    for row in case["fai"].decode().splitlines():
        f = row.split("\t")
        fai[f[0]] = int(f[1])
    depth = {}
    for row in case["depth"].decode().splitlines():
        f = row.split("\t")
        depth[f[0]] = (int(f[1]), int(f[2]))
    return fai, depth


def corrected_dup(case, trace=None):
    """the model: case (fai, cycle, final, before_cut, depth: bytes; min_len) -> (the bytes of final.txt, the bytes of stdout)"""
    trace = set() if trace is None else trace
    fai, depth = parse_inputs(case)
    before = {}
    for k, row in enumerate(case["before_cut"].decode().splitlines(), 1):
        parts = row.strip().split(":")
        if len(parts) != 2:
            raise Rejected("before_cut", k, "not one ':'")
        if parts[0]:
            key, value = parts[0].split(), parts[1].split()
            check_tokens(key, fai, "before_cut", k)
            check_tokens(value, fai, "before_cut", k)
            before["\t".join(key)] = "\t".join(value)
    originals, corrected = [], []
    cycle_rows = case["cycle"].decode().splitlines()
    if not cycle_rows:
        trace.add("no_cycle_line")
    for k, row in enumerate(cycle_rows, 1):
        tokens = row.split()
        if not tokens:
            raise Rejected("cycle", k, "a blank line")
        check_tokens(tokens, fai, "cycle", k)
        originals.append(tokens)
        corrected.append(correct_cycle(tokens, fai, depth, trace))
    kept_cycles = [corrected[k] for k in greedy_paths(corrected, fai, trace)]
    paths = [list(p) for p in kept_cycles]
    original_sets = [set(base_of(t) for t in o) for o in originals]
    for k, row in enumerate(case["final"].decode().splitlines(), 1):
        tokens = row.split()
        if not tokens:
            continue
        check_tokens(tokens, fai, "final", k)
        key = "\t".join(tokens)
        if key in before:
            trace.add("before_cut_replace")
            tokens = before[key].split()
        if set(base_of(t) for t in tokens) in original_sets:
            trace.add("base_set_skip")
            continue
        paths.append(tokens)
    back = {v: k for k, v in before.items()}
    survivors = [paths[k] for k in greedy_paths(paths, fai, trace)]
    first = [p for p in survivors if p in kept_cycles]
    second = []
    for p in survivors:
        if p not in kept_cycles:
            joined = "\t".join(p)
            if joined in back:
                trace.add("map_back")
                p = back[joined].split("\t")
            second.append(p)
    out, stdout = [], []
    for p in first + second:
        q, warn = quota(p, trace)
        stdout += warn
        n = path_len(q)
        if n == case["min_len"]:
            trace.add("at_min_len")
        if n == case["min_len"] + 1:
            trace.add("at_min_len_plus_1")
        if n > case["min_len"]:
            out.append("\t".join(q) + "\n")
    return "".join(out).encode(), "".join(stdout).encode()


# ---- the cases ----------------------------------------------------------------------------------------------------------------------


def edge(uid, length, cov):
    return f"EDGE_{uid}_length_{length}_cov_{cov}"


def make_case(contigs, cycles, finals, before=(), depth=None, min_len=0):
    """contigs: (name, .fai length) in order; cycles, finals: token lists; before: (key tokens, value tokens); depth: name -> (sum,
    covered), a contig that is absent is unknown to the BAM"""
    depth = {} if depth is None else depth
    return dict(fai="".join(f"{n}\t{ln}\t0\t60\t61\n" for n, ln in contigs).encode(),
                cycle="".join("\t".join(c) + "\n" for c in cycles).encode(),
                final="".join("\t".join(f) + "\n" for f in finals).encode(),
                before_cut="".join("\t".join(k) + ":" + "\t".join(v) + "\n" for k, v in before).encode(),
                depth="".join(f"{n}\t{s}\t{c}\n" for n, (s, c) in depth.items()).encode(), min_len=int(min_len))


def hand_cases():
    A, B, C, D, E, F, G = (edge(k + 1, ln, cov) for k, (ln, cov) in enumerate(((900, "10.0"), (100, "10.5"), (300, "9.5"), (450, "30.25"), (50, "11.0"), (8999, "10.0"),
                                                                               (1001, "10.0"))))
    X = "CTG001"
    contigs = [(A, 900), (B, 100), (C, 300), (D, 450), (E, 50), (F, 8999), (G, 1001), (X, 70)]
    flat = {n: (10 * ln, ln) for n, ln in contigs}
    cases = {}
    cases["no_cycles"] = make_case(contigs, [], [[A + "+", B + "-"], [C + "+", D + "+", X + "+"]], depth=flat)
    cases["border"] = make_case(contigs, [[A + "+", B + "+", C + "+", A + "+"], [C + "+", D + "-", E + "+", C + "+", D + "-"]], [[E + "+", F + "+"]], depth=flat)
    cases["merge"] = make_case(contigs, [[B + "+", A + "+", C + "+", A + "-", D + "+", A + "+", C + "+"]], [[F + "+", G + "+"]], depth=flat)
    deep = dict(flat)
    deep[B] = (40 * 100, 100)
    deep[C] = (90 * 300, 300)
    cases["tandem_by_depth"] = make_case(contigs, [[A + "+", B + "+", B + "+", B + "+", D + "+"]], [[F + "+"]], depth=deep)
    cases["two_units"] = make_case(contigs, [[A + "+", B + "+", B + "+", D + "+", C + "-", E + "+", C + "-", E + "+", C + "-", E + "+", G + "+"]], [[F + "+"]], depth=deep)
    # A border of 1 rotates this to b b c d c d b b E: the unit [b] takes everything from the first b b to the last, [c d][c d] with it.
    # What comes out depends on the order of the two units, which the script leaves to a set of strings and the rules to discovery
    # (a declared deviation): the ids 111, 611 and 1111 are ones where that set yields the discovery order under hash seeds 0 - 3.
    b, c, d = edge(111, 100, "10.5"), edge(611, 300, "9.5"), edge(1111, 450, "30.25")
    own = [(b, 100), (c, 300), (d, 450), (E, 50), (F, 8999)]
    cases["doubled_gone"] = make_case(own, [[b + "+", c + "+", d + "+", c + "+", d + "+", b + "+", b + "+", E + "+", b + "+"]], [[F + "+"]],
                                      depth={n: (10 * ln, ln) for n, ln in own})
    cases["collapse"] = make_case(contigs, [], [[C + "+", B + "+", D + "+", B + "+", D + "+"]], depth=flat)
    cases["both_strands"] = make_case(contigs, [[A + "+", B + "+", A + "-", B + "+", C + "+"], [D + "+", B + "-", B + "+", B + "-", B + "+", E + "+"]], [[F + "-", G + "+"]], depth=deep)
    gaps = {k: v for k, v in deep.items() if k != C}
    gaps[D] = (0, 0)
    cases["unknown_and_bare"] = make_case(contigs, [[A + "+", C + "+", C + "+", D + "+", D + "+", B + "+"]], [[F + "+", X + "-"]], depth=gaps)
    cases["mean_zero"] = make_case(contigs, [[A + "+", B + "+", B + "+", B + "+", C + "+"]], [[F + "+"]], depth={n: (0, ln) for n, ln in contigs})
    cases["before_cut"] = make_case(contigs, [[A + "+", B + "+", C + "+"]], [[F + "+", G + "+"], [D + "+", E + "+"], [A + "-", C + "-", B + "-", B + "+"]],
                                    before=[([F + "+", G + "+"], [F + "+"]), ([D + "+", E + "+"], [D + "+", X + "+"]), ([X + "+"], [E + "+"]), ([D + "+", E + "+"], [D + "+", X + "-"])], depth=flat)
    cases["ratio"] = make_case(contigs, [], [[A + "+", B + "+"], [A + "+", C + "+", E + "+"], [F + "+", G + "+"], [F + "+", D + "+", C + "+", B + "+"], [D + "+", E + "+"], [E + "-", D + "-"]],
                               depth=flat)
    cases["ratio_under"] = make_case(contigs, [], [[F + "+", G + "+"], [F + "+", A + "+", B + "+", E + "+", X + "+"]], depth=flat)
    cases["hub"] = make_case(contigs, [], [[A + "+", D + "+", B + "+", D + "+", C + "+", D + "+", A + "+", A + "+", B + "+", X + "+"]], depth=flat)
    cases["budget"] = make_case(contigs, [], [[A + "+", B + "+", A + "+", A + "+", C + "+", A + "-", E + "+"], [F + "+", F + "+", G + "+", F + "+", F + "+"]], depth=flat)
    cases["only_plain"] = make_case(contigs, [], [[X + "+", X + "-"]], depth=flat)
    cases["min_len"] = make_case(contigs, [], [[A + "+", B + "+"], [F + "+", E + "+", X + "+"], [C + "+"]], depth=flat, min_len=1000)
    cases["min_len_plus_1"] = make_case(contigs, [], [[A + "+", B + "+"], [F + "+", E + "+"], [C + "+"]], depth=flat, min_len=999)
    odd = [(edge(1, 500, "3.0"), 777), (edge(2, 40, "3..5"), 4000), (edge(3, 60, "."), 60), (edge(4, 80, "0.0"), 80), (edge(5, 90, "0"), 90)]
    o = [n for n, _ in odd]
    cases["odd_names"] = make_case(odd, [[o[0] + "+", o[3] + "+", o[3] + "+", o[4] + "-"]], [[o[0] + "+", o[1] + "+", o[2] + "-"], [o[3] + "+", o[4] + "+"], [o[1] + "-"]],
                                   depth={n: (5 * ln, ln) for n, ln in odd})
    return cases


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 10))
    contigs = []
    for k in range(n):
        ln = int(rng.choice([40, 55, 100, 100, 250, 700, 1500, 4000]))
        if rng.random() < 0.15:
            contigs.append((f"CTG{k:03d}", ln))
        else:
            stated = ln if rng.random() < 0.8 else int(rng.integers(1, 3000))
            contigs.append((edge(k + 1, stated, str(rng.choice(["4.0", "5.5", "10.25", "11.0", "12.5", "24.0", "60.0", "7"]))), ln))
    names = [c[0] for c in contigs]
    depth = {}
    for name, ln in contigs:
        u = rng.random()
        if u < 0.1:
            continue
        cov = 0 if u < 0.2 else int(rng.integers(1, ln + 1))
        depth[name] = (cov * int(rng.choice([0, 3, 10, 11, 25, 60])) + (int(rng.integers(0, cov)) if cov else 0), cov)

    def tok():
        return names[int(rng.integers(0, n))] + "+-"[int(rng.integers(0, 2))]

    def walk(lo, hi):
        return [tok() for _ in range(int(rng.integers(lo, hi + 1)))]

    cycles = []
    for _ in range(int(rng.integers(0, 4))):
        kind = rng.random()
        unit = walk(1, 3)
        if kind < 0.5:
            c = walk(1, 3) + unit * int(rng.integers(2, 5)) + walk(0, 3)
        elif kind < 0.7:
            head = walk(1, 2)
            c = head + walk(1, 4) + head
        else:
            c = walk(2, 9)
        cycles.append(c)
    finals = [walk(1, 7) for _ in range(int(rng.integers(1, 5)))]
    if cycles and rng.random() < 0.4:
        c = cycles[int(rng.integers(0, len(cycles)))]
        finals.insert(int(rng.integers(0, len(finals) + 1)), [c[int(q)] for q in rng.permutation(len(c))])
    before = []
    if rng.random() < 0.5:
        before.append((finals[int(rng.integers(0, len(finals)))], walk(1, 5)))
    total = sum(path_len(f) for f in finals) // max(1, len(finals))
    return make_case(contigs, cycles, finals, before, depth, int(rng.choice([0, 0, 100, total, 10 ** 7])))


N_RANDOM = 48


def golden_inputs():
    cases = hand_cases()
    for seed in range(N_RANDOM):
        cases[f"random_{seed:02d}"] = random_case(9000 + seed)
    return cases
