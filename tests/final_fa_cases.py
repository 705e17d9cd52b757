"""make_final_fa restated in plain Python, and the inputs of its tests (no tests here; `python -m tests.final_fa_cases` checks the
restatement against hand-written cases).

The rules are DESIGN.md 8's.  `cycle_interval` is the LITERAL form of the cycle test: the loop over every 0 <= i <= j < L with the
sums taken afresh for every interval, no pruning, the first interval of least trimmed length kept.  `cycle_interval_pruned` is the
same decision with the prefix sums used first; it is there for paths too long for the literal form and is held to it on random
cases (tests/test_host_final_fa_rules.py).  The graph rules, the decision, the order, the numbering, the separators and the
headers are pinned by tests/golden/final_fa_cases.npz, which holds what the reference's script itself wrote for `golden_inputs()`;
the FASTA reader (tests/path_fasta_cases.py: the project's index) and the complement table are not -- Biopython is absent."""
import re

import numpy as np

from tests import path_fasta_cases as pc

BAD_BYTE = b"a byte other than TAB, space and 0x21-0x7E (a CR is allowed directly before the LF)"
BAD_ORIENTATION = b"an orientation field of a JUNC line that is neither '+' nor '-'"
NO_LENGTH = b"a node without 'length_' and 1 to 12 digits behind it"
TOO_MANY_TOKENS = b"a path of 2^20 tokens or more"
MAX_TOKENS = 1 << 20
SEP = b"N" * 50


class Fault(Exception):
    """a file outside the grammar: which of the inputs ('paths', 'graph', 'fasta'), the 1-based line, the reason"""

    def __init__(self, which, line, reason):
        super().__init__(f"{which}: line {line}: {reason!r}")
        self.which, self.line, self.reason = which, line, reason


# ---- lines and tokens -------------------------------------------------------------------------------------------------------------

def lines_of(text: bytes):
    """-> [(1-based line number, the line without its LF and without a CR directly before it)]"""
    if not text:
        return []
    raw = text.split(b"\n")
    last_has_lf = text.endswith(b"\n")
    if last_has_lf:
        raw.pop()
    out = []
    for k, line in enumerate(raw):
        if (k + 1 < len(raw) or last_has_lf) and line.endswith(b"\r"):
            line = line[:-1]
        out.append((k + 1, line))
    return out


def bytes_ok(line: bytes) -> bool:
    return all(c == 9 or 0x20 <= c <= 0x7e for c in line)


def fields(line: bytes):
    return [f for f in re.split(rb"[ \t]+", line) if f]


def length_of(name: bytes):
    """the digits behind the first 'length_' that has digits behind it; None without one, or with more than 12 digits"""
    m = re.search(rb"length_([0-9]+)", name)
    if not m or len(m.group(1)) > 12:
        return None
    return int(m.group(1))


def base_of(token: bytes) -> bytes:
    return token.rstrip(b"+-")


def flip(o: bytes) -> bytes:
    return b"+" if o == b"-" else b"-"


def query_of(token: bytes) -> bytes:
    """what is looked up in the assembly: 'ref' removed, the last byte as the strand ('-' or, for anything else, '+')"""
    t = token.replace(b"ref", b"")
    return t if not t or t.endswith(b"-") else t[:-1] + b"+"


def parse_graph(text: bytes):
    """-> the arcs in file order, [(source, destination)], a line's own arc before its conjugate"""
    arcs = []
    for no, line in lines_of(text):
        if not bytes_ok(line):
            raise Fault("graph", no, BAD_BYTE)
        if not line.startswith(b"JUNC"):
            continue
        f = fields(line)
        if len(f) < 5:
            continue
        if f[2] not in (b"+", b"-") or f[4] not in (b"+", b"-"):
            raise Fault("graph", no, BAD_ORIENTATION)
        if length_of(f[1]) is None or length_of(f[3]) is None:
            raise Fault("graph", no, NO_LENGTH)
        arcs.append((f[1] + f[2], f[3] + f[4]))
        arcs.append((f[3] + flip(f[4]), f[1] + flip(f[2])))
    return arcs


def parse_paths(text: bytes):
    """-> [(1-based line number, [token, ...])] of the lines that are paths"""
    out = []
    for no, line in lines_of(text):
        if not bytes_ok(line):
            raise Fault("paths", no, BAD_BYTE)
        if b"all" in line:
            continue
        f = fields(line)
        if not f:
            continue
        if len(f) >= MAX_TOKENS:
            raise Fault("paths", no, TOO_MANY_TOKENS)
        if any(length_of(t) is None for t in f):
            raise Fault("paths", no, NO_LENGTH)
        out.append((no, f))
    return out


def hexed(b: bytes) -> bytes:
    return b.hex().encode() if b else b"-"


def dump_graph(text: bytes):
    """what `final_tokens_selftest graph` prints, as lines"""
    try:
        arcs = parse_graph(text)
    except Fault as f:
        return [b"F %d %s" % (f.line, f.reason)]
    return [b"A %s %d %s %d" % (hexed(s), length_of(s), hexed(d), length_of(d)) for s, d in arcs]


def dump_paths(text: bytes):
    """what `final_tokens_selftest paths` prints, as lines"""
    try:
        paths = parse_paths(text)
    except Fault as f:
        return [b"F %d %s" % (f.line, f.reason)]
    out = []
    for no, toks in paths:
        out.append(b"L %d %d" % (no, len(toks)))
        out += [b"T %s %d %s %s" % (hexed(t), length_of(t), hexed(base_of(t)), hexed(query_of(t))) for t in toks]
    return out


# ---- the cycle test ---------------------------------------------------------------------------------------------------------------

def cycle_interval(node, base, length, arcs, trim_threshold, min_cycle_length):
    """The literal form over one path: node / base / length per token (anything hashable; equal bases have equal lengths), arcs a
    set of (source node, destination node) -> (i, j) of the kept interval or (-1, -1)."""
    L = len(node)
    valid = []
    for i in range(L):
        for j in range(i, L):
            trimmed = sum(length[:i]) + sum(length[j + 1:])
            if trimmed > trim_threshold:
                continue
            if (node[j], node[i]) not in arcs:
                continue
            first_of_base = {}
            for k in range(i, j + 1):
                first_of_base.setdefault(base[k], length[k])
            if sum(first_of_base.values()) >= min_cycle_length:
                valid.append((trimmed, i, j))
    if not valid:
        return -1, -1
    valid.sort(key=lambda v: v[0])                                # (stable: among equals the first in (i, j) order)
    return valid[0][1], valid[0][2]


def cycle_interval_pruned(node, base, length, arcs, trim_threshold, min_cycle_length):
    """the same decision: i bounded from above and j from below by the prefix sums, the distinct-base sum carried along j"""
    L = len(node)
    if L == 0 or trim_threshold < 0:
        return -1, -1
    pre = [0] * (L + 1)
    for k in range(L):
        pre[k + 1] = pre[k] + length[k]
    total = pre[L]
    best = None
    for i in range(L):
        if pre[i] > trim_threshold:
            break
        jmin = L - 1
        while jmin > i and total - pre[jmin] <= trim_threshold - pre[i]:      # (j = jmin - 1 trims total - pre[jmin] behind it)
            jmin -= 1
        seen, uniq = set(), 0
        for j in range(i, L):
            if base[j] not in seen:
                seen.add(base[j])
                uniq += length[j]
            if j >= jmin and uniq >= min_cycle_length and (node[j], node[i]) in arcs:
                key = (pre[i] + total - pre[j + 1], i, j)
                if best is None or key < best:
                    best = key
    return (best[1], best[2]) if best else (-1, -1)


# ---- the whole tool ---------------------------------------------------------------------------------------------------------------

_COMP = bytes.maketrans(b"ACGTRYKMBDHVacgtrykmbdhv", b"TGCAYRMKVHDBtgcayrmkvhdb")      # S, W, N and every other byte stay


def reverse_complement(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def read_fasta(fasta: bytes):
    """-> {name: sequence} by the project's index; a fault of the index, or a name's second record, raises Fault"""
    recs, code, line = pc.fasta_index(fasta)
    if code:
        raise Fault("fasta", line, code)
    seqs = {}
    for r in recs:
        if r["name"] in seqs:
            raise Fault("fasta", fasta.count(b"\n", 0, r["name_off"]) + 1, b"duplicate")
        seqs[r["name"]] = pc.sequence_of(fasta, r)
    return seqs


def final_fa(paths: bytes, graph: bytes, fasta: bytes, prefix: bytes, fasta_name: bytes, out_name: bytes, trim_threshold=300, min_cycle_length=10000,
             decide=cycle_interval):
    """-> (the output file's bytes, stderr)"""
    arcs = set(parse_graph(graph))
    plist = parse_paths(paths)
    seqs = read_fasta(fasta)
    cycles, linear = [], []
    for _, toks in plist:
        i, j = decide(toks, [base_of(t) for t in toks], [length_of(t) for t in toks], arcs, trim_threshold, min_cycle_length)
        if i >= 0:
            cycles.append(toks[i:j + 1])
        else:
            linear.append(toks)
    out, err, count = [], [], 0
    for group, tag in ((cycles, b"cycle"), (linear, b"linear")):
        for toks in group:
            seq = b""
            for t in toks:
                q = query_of(t)
                name, rev = q[:-1], q.endswith(b"-")
                if name not in seqs:
                    err.append(b"Warning: Node '%s' not found in %s\n" % (name, fasta_name))
                    continue
                s = reverse_complement(seqs[name]) if rev else seqs[name]
                seq = s if seq == b"" else seq + SEP + s
            if seq != b"":
                count += 1
                out.append(b">%s_phage_%d_%s\n%s\n" % (prefix, count, tag, seq))
    err.append(b"Total circular paths found: %d\nTotal linear paths found: %d\nFasta successfully written to: %s\n\n" % (len(cycles), len(linear), out_name))
    return b"".join(out), b"".join(err)


# ---- builders ---------------------------------------------------------------------------------------------------------------------

def node(k: int, length: int, extra: bytes = b"") -> bytes:
    return b"EDGE_%d_length_%d_cov_%d.5%s" % (k, length, k % 7 + 1, extra)


def junc(a: bytes, oa: bytes, b: bytes, ob: bytes, tail: bytes = b" 12 0 3") -> bytes:
    return b"JUNC " + a + b" " + oa + b" " + b + b" " + ob + tail + b"\n"


def fasta_for(rng, names_lengths, width=60, eol=b"\n"):
    """records named as given with sequences of the given lengths (the FASTA's own lengths need not be the names')"""
    return pc.fasta_text([(nm, pc.random_seq(rng, n)) for nm, n in names_lengths], width, eol)


def _hand_case(rng):
    """one assembly, several paths: exact cycles, trims at both ends, the tie, a conjugate-only arc, repeats, tokens that are no record"""
    n = {k: node(k, l) for k, l in ((1, 6000), (2, 5000), (3, 100), (4, 100), (5, 200), (6, 101), (7, 9999), (8, 1), (9, 4000), (10, 0), (11, 300))}
    fasta = fasta_for(rng, [(n[k], 20 + 3 * k) for k in (1, 2, 3, 4, 5, 6, 7, 8, 9)] + [(n[10], 0), (n[11] + b" described", 75), (b"EDGE_12_length_120", 17)])
    graph = (b"# made by hand\nSEG " + n[1] + b" 5 1\n" +
             junc(n[2], b"+", n[1], b"+") +                      # closes 1+ 2+
             junc(n[1], b"-", n[2], b"+") +                      # conjugate: 2- -> 1+
             junc(n[9], b"+", n[9], b"+") +                      # a self-arc
             junc(n[7], b"+", n[8], b"-") + junc(n[8], b"-", n[7], b"+") +
             b"JUNC " + n[3] + b" + " + n[4] + b"\n" +             # four fields: nothing
             b"JUNCTION\t" + n[2] + b"\t-\t" + n[2] + b"\t-\textra\n" +   # begins with JUNC: counts; TABs
             junc(n[2], b"+", n[2], b"+") + junc(n[2], b"+", n[2], b"+"))   # twice the same
    paths = (b"all paths follow\n"
             b"\n"
             + n[1] + b"+ " + n[2] + b"+\n"                                          # an exact cycle
             + n[3] + b"+ " + n[1] + b"+ " + n[2] + b"+ " + n[4] + b"+\n"             # 100 trimmed in front, 100 behind
             + n[3] + b"+\t" + n[1] + b"+\t\t" + n[2] + b"+  " + n[5] + b"+\r\n"      # front 100 + back 200 = 300: at the threshold
             + n[3] + b"+ " + n[1] + b"+ " + n[2] + b"+ " + n[5] + b"+ " + n[8] + b"+\n"   # 301: linear
             + n[2] + b"- " + n[1] + b"+\n"                                          # the arc 2- -> 1+ exists only as a conjugate
             + n[2] + b"+ " + n[2] + b"+ " + n[2] + b"-\n"                            # one base three times: 5000 < the minimum
             + n[9] + b"+\n"                                                        # a self-arc, 4000 < the minimum
             + b"  " + n[7] + b"+ " + n[8] + b"-  \n"                                # 9999 + 1: at the minimum
             + b"overall_length_5+\n"                                               # holds 'all'
             + n[1] + b"+ EDGE_77_length_5000+ " + n[2] + b"+\n"                      # the middle token is no record
             + b"EDGE_77_length_5000- " + n[1] + b"- EDGE_78_length_1+\n"            # the first and the last are none
             + b"EDGE_77_length_5000+ EDGE_78_length_1-\n"                          # nothing found: no record, no number
             + n[10] + b"+ " + n[3] + b"- " + n[10] + b"- " + n[4] + b"+\n"           # an empty first record: no separator behind it
             + b"ref" + n[5] + b"ref+ EDGE_12_length_120x " + n[11] + b"-ref\n"       # 'ref' removed; a last byte that is no strand
             + n[6] + b"+")                                                         # no LF at the end
    return paths, graph, fasta


def _tie_case(rng):
    """front-trim 100 versus back-trim 100: both [1, L-1] and [0, L-2] pass with trimmed = 100; the first in (i, j) order is (0, L-2)"""
    a, b, c, d = node(1, 100), node(2, 7000), node(3, 7000), node(4, 100)
    graph = junc(d, b"+", b, b"+") + junc(c, b"+", a, b"+")          # 4+ -> 2+ closes [1, 3]; 3+ -> 1+ closes [0, 2]
    paths = b" ".join(x + b"+" for x in (a, b, c, d)) + b"\n"
    return paths, graph, fasta_for(rng, [(a, 11), (b, 12), (c, 13), (d, 14)])


def _random_case(rng, n_nodes=12, n_paths=30, max_len=9):
    lens = [int(rng.choice([0, 1, 50, 100, 150, 299, 300, 301, 2000, 5000, 9000])) for _ in range(n_nodes)]
    names = [node(k, l) for k, l in enumerate(lens)]
    strands = (b"+", b"-")
    graph = b"".join(junc(names[int(rng.integers(n_nodes))], strands[int(rng.integers(2))], names[int(rng.integers(n_nodes))], strands[int(rng.integers(2))])
                     for _ in range(3 * n_nodes))
    paths = b"".join(b" ".join(names[int(rng.integers(n_nodes))] + strands[int(rng.integers(2))] for _ in range(int(rng.integers(1, max_len + 1)))) + b"\n"
                     for _ in range(n_paths))
    fasta = fasta_for(rng, [(nm, int(rng.integers(0, 90))) for k, nm in enumerate(names) if k % 5 != 4], width=int(rng.integers(7, 70)))
    return paths, graph, fasta


def golden_inputs():
    """{case: (paths, graph, fasta, prefix, [option words])}: every one inside the grammar of DESIGN.md 8"""
    rng = np.random.default_rng(20260)
    cases = {}
    cases["hand"] = _hand_case(rng) + (b"S01", [])
    cases["hand_crlf_fasta"] = cases["hand"][:2] + (cases["hand"][2].replace(b"\n", b"\r\n"), b"sample_2", [])
    cases["tie"] = _tie_case(rng) + (b"T", [])
    cases["tie_threshold_99"] = _tie_case(rng) + (b"T", [b"--trim_threshold", b"99"])
    cases["tie_minimum_14001"] = _tie_case(rng) + (b"T", [b"--min_cycle_length=14001"])
    cases["threshold_0"] = _hand_case(rng) + (b"Z", [b"--trim_threshold=0", b"--min_cycle_length", b"1"])
    cases["threshold_negative"] = _hand_case(rng) + (b"Z", [b"--trim_threshold=-1", b"--min_cycle_length=0"])
    cases["no_paths"] = (b"all\n\n", cases["hand"][1], cases["hand"][2], b"E", [])
    cases["no_arcs"] = (cases["hand"][0], b"SEG only\n", cases["hand"][2], b"E", [])
    for k in range(6):
        cases[f"random_{k}"] = _random_case(rng) + (b"r%d" % k, [[], [b"--min_cycle_length", b"5000"], [b"--trim_threshold=1000", b"--min_cycle_length=300"]][k % 3])
    return cases


def options_of(words):
    """the option words of a case -> (trim_threshold, min_cycle_length)"""
    thr, mn, k = 300, 10000, 0
    while k < len(words):
        w = words[k]
        name, eq, val = w.partition(b"=")
        if not eq:
            k += 1
            val = words[k]
        if name == b"--trim_threshold":
            thr = int(val)
        else:
            assert name == b"--min_cycle_length"
            mn = int(val)
        k += 1
    return thr, mn


def faulty_inputs():
    """{case: (which file, text, 1-based line, reason)}: each declared fault of the two small files alone"""
    p, g, _ = _hand_case(np.random.default_rng(1))
    pl, gl = p.split(b"\n"), g.split(b"\n")
    def with_line(lines, k, new):
        return b"\n".join(lines[:k] + [new] + lines[k + 1:])
    return {
        "paths_high_byte": ("paths", with_line(pl, 3, pl[3][:9] + b"\xc3\xa9" + pl[3][9:]), 4, BAD_BYTE),
        "paths_high_byte_in_skipped_line": ("paths", with_line(pl, 0, b"all \x80"), 1, BAD_BYTE),
        "paths_cr_inside": ("paths", with_line(pl, 5, pl[5][:4] + b"\r" + pl[5][4:]), 6, BAD_BYTE),
        "paths_vertical_tab": ("paths", with_line(pl, 2, pl[2].replace(b" ", b"\x0b", 1)), 3, BAD_BYTE),
        "paths_no_length": ("paths", with_line(pl, 6, pl[6] + b" EDGE_5_len_7+"), 7, NO_LENGTH),
        "paths_length_without_digits": ("paths", with_line(pl, 2, b"EDGE_1_length_+"), 3, NO_LENGTH),
        "paths_thirteen_digits": ("paths", with_line(pl, 2, b"EDGE_1_length_1234567890123+"), 3, NO_LENGTH),
        "paths_two_faults": ("paths", with_line(with_line(pl, 9, b"nolen+").split(b"\n"), 4, b"nolen-"), 5, NO_LENGTH),
        "graph_bad_orientation": ("graph", with_line(gl, 2, gl[2].replace(b" + ", b" * ", 1)), 3, BAD_ORIENTATION),
        "graph_orientation_two_bytes": ("graph", with_line(gl, 3, gl[3].replace(b" - ", b" -- ", 1)), 4, BAD_ORIENTATION),
        "graph_no_length": ("graph", with_line(gl, 4, b"JUNC EDGE_9 + EDGE_9_length_4000_cov_3.5 + 1"), 5, NO_LENGTH),
        "graph_high_byte_in_comment": ("graph", with_line(gl, 0, b"# caf\xe9"), 1, BAD_BYTE),
        "graph_nul": ("graph", with_line(gl, 5, gl[5] + b"\x00"), 6, BAD_BYTE),
    }


TOKEN_HAND = [b"", b"\n", b"\r\n", b" \t \n", b"length_5", b"a_length_12+\tb_length_0-", b"x_length_1+ \r\n\r\ny_length_2--+\r\n", b"length_length_7+\n",
              b"length_x_length_9\n", b"reflength_3ref-ref\n", b"rreffef_length_4+\n", b"wall_length_1+\nlength_2+\n", b"length_123456789012-\n",
              b"JUNC a_length_1 + b_length_2 -\n", b"JUNCa_length_1 + b_length_2 - 7\nJUNC a_length_1 + b_length_2\n junc\n JUNC a_length_1 + b_length_2 - 7\n",
              b"JUNC\ta_length_1\t+\tb_length_2\t-\r\nJUNC a_length_1 - a_length_1 +", b"length_5\r", b"length_5+\r\r\n"]


def hand_checks():
    """the restatement against cases worked by hand"""
    assert lines_of(b"a\r\nb\r") == [(1, b"a"), (2, b"b\r")] and lines_of(b"\n") == [(1, b"")] and lines_of(b"") == []
    assert length_of(b"EDGE_1_length_280_cov_3") == 280 and length_of(b"length_x_length_9") == 9 and length_of(b"length_") is None
    assert length_of(b"length_0123456789012") is None and length_of(b"length_012345678901") == 12345678901
    assert base_of(b"a+-+") == b"a" and base_of(b"a+b") == b"a+b" and query_of(b"refa_refb+") == b"a_b+" and query_of(b"abc") == b"ab+" and query_of(b"ab-") == b"ab-"
    assert parse_graph(b"JUNC a_length_1 + b_length_2 - x\n") == [(b"a_length_1+", b"b_length_2-"), (b"b_length_2+", b"a_length_1-")]
    assert parse_paths(b"all\n  \nlength_1+  length_2-\t\n") == [(3, [b"length_1+", b"length_2-"])]
    # the cycle test on integers: nodes 0 .. 3 with lengths 100, 7000, 7000, 100
    lens, ids = [100, 7000, 7000, 100], [0, 1, 2, 3]
    for f in (cycle_interval, cycle_interval_pruned):
        assert f(ids, ids, lens, {(3, 1), (2, 0)}, 300, 10000) == (0, 2)          # the tie: the first in (i, j) order
        assert f(ids, ids, lens, {(3, 1)}, 300, 10000) == (1, 3)
        assert f(ids, ids, lens, {(3, 0), (2, 0), (3, 1)}, 300, 10000) == (0, 3)   # nothing trimmed wins
        assert f(ids, ids, lens, {(2, 1)}, 200, 10000) == (1, 2) and f(ids, ids, lens, {(2, 1)}, 199, 10000) == (-1, -1)
        assert f(ids, ids, lens, {(2, 1)}, 200, 14000) == (1, 2) and f(ids, ids, lens, {(2, 1)}, 200, 14001) == (-1, -1)
        assert f([0, 1, 4], [0, 1, 0], [5, 6, 5], {(4, 0)}, 0, 11) == (0, 2) and f([0, 1, 4], [0, 1, 0], [5, 6, 5], {(4, 0)}, 0, 12) == (-1, -1)
        assert f([], [], [], {(0, 0)}, 300, 0) == (-1, -1) and f([7], [7], [0], {(7, 7)}, 0, 0) == (0, 0) and f([7], [7], [0], {(7, 7)}, -1, 0) == (-1, -1)
    p, g, fa = _tie_case(np.random.default_rng(5))
    out, err = final_fa(p, g, fa, b"T", b"asm.fasta", b"out.fasta")
    seqs = read_fasta(fa)
    a, b, c = (seqs[node(k, l)] for k, l in ((1, 100), (2, 7000), (3, 7000)))
    assert out == b">T_phage_1_cycle\n" + a + SEP + b + SEP + c + b"\n", out
    assert err == b"Total circular paths found: 1\nTotal linear paths found: 0\nFasta successfully written to: out.fasta\n\n"
    out, err = final_fa(b"x_length_1- y_length_2+ z_length_3x\n", b"", b">x_length_1\nACGTRYKMBDHVSWN\nacgtn\n>z_length_3\n\n>w\nTT\n", b"P", b"f.fa", b"o.fa")
    assert out == b">P_phage_1_linear\nnacgtNWSBDHVKMRYACGT" + SEP + b"\n" and err.startswith(b"Warning: Node 'y_length_2' not found in f.fa\nTotal circular paths found: 0\n"), (out, err)
    for name, (paths, graph, fasta, prefix, words) in golden_inputs().items():
        thr, mn = options_of(words)
        assert final_fa(paths, graph, fasta, prefix, b"a", b"o", thr, mn) == final_fa(paths, graph, fasta, prefix, b"a", b"o", thr, mn, cycle_interval_pruned), name
    for name, (which, text, line, reason) in faulty_inputs().items():
        try:
            (parse_paths if which == "paths" else parse_graph)(text)
            raise AssertionError(name + " must raise")
        except Fault as f:
            assert (f.which, f.line, f.reason) == (which, line, reason), (name, f.line, f.reason)


if __name__ == "__main__":
    hand_checks()
    print("final_fa_cases: the restatement agrees with the hand-worked cases")
