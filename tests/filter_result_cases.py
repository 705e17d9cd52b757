"""filter_result in plain Python, in literal form: what the reference's share/palace/scripts/filter_result.py does, restated line by
line from reading and running it (DESIGN.md 8 states the rules and the declared deviations), and the seeded catalogue of inputs the
golden file tests/golden/filter_result_cases.npz is made of -- every input inside the strict grammar, so the reference exits 0 on it.

  filter_result(...)        the whole command: FASTA bytes, the tagged stdout lines, the cycle file's lines (in OUR declared order:
                            first appearance), the class of every path and a count of every branch taken;
  path_class(...)           the class byte of a path from its facts -- the integer form the device decides (checked against the
                            literal form on every path of the catalogue by tests/test_host_filter_result_rules.py);
  blast_line / dump_blast   the grammar of one line of the BLAST table, as csrc/blast_line.hpp states it;
  blast_groups(...)         the groups of a table as integers (lines, groups, flagged names, the first fault);
  identity_cuts(...)        the search of the seven cuts;
  first_of_equal(...)       the first-occurrence rule over equal code sequences, per class bit;
  golden_inputs()           name -> (fasta, paths, blast, ratio text, hits, scores);
  faulty_inputs()           name -> (which file, the inputs with that file replaced, line, reason).

`python -m tests.filter_result_cases` checks the restatement against a few hand-written cases."""
import collections
import re

import numpy as np

WRITE, PLAIN, SELFGENE, CYCLEGENE, CYCLESCORE, GENESCORE = 1, 2, 4, 8, 16, 32
REC_GENE, REC_S07, REC_S09, REC_BLAST = 1, 2, 4, 8
TAG_SELF, TAG_CYCLE = 1, 2
E_COLUMNS, E_NAME, E_IDENTITY, E_LENGTH, E_QUERY, E_QEMPTY = 1, 2, 3, 4, 5, 6
BLAST_REASON = {E_COLUMNS: b"fewer than four columns", E_NAME: b"an empty query or subject",
                E_IDENTITY: b"an identity that is not digits[.digits] with at most 3 and 6 digits", E_LENGTH: b"an alignment length that is not 1-10 digits",
                E_QUERY: b"the query is no record of the FASTA", E_QEMPTY: b"the query's record has no bases"}
RESERVED = (b"ref", b"self", b"gene", b"score", b"cycle")
TAGGED = (b"selfgene", b"cyclegene", b"cyclescore", b"genescore")
_COMP = bytes.maketrans(b"ACGTRYKMBDHVacgtrykmbdhv", b"TGCAYRMKVHDBtgcayrmkvhdb")
_IDENTITY = re.compile(rb"[0-9]{1,3}(\.[0-9]{1,6})?\Z")
_LENGTH = re.compile(rb"[0-9]{1,10}\Z")
_NUMBER = re.compile(rb"-?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?\Z")


class Fault(Exception):
    def __init__(self, which, line, reason):
        super().__init__(which, line, reason)
        self.which, self.line, self.reason = which, line, reason


def file_lines(text: bytes):
    """the lines of a file as Python iterates over it, each with its LF where it has one"""
    return re.findall(rb"[^\n]*\n|[^\n]+\Z", text)


def parse_fasta(fasta: bytes):
    """name -> sequence, in file order: the first word of the header line, the lines up to the next header stripped and joined"""
    out, name, parts = {}, None, []
    for line in file_lines(fasta):
        if line.startswith(b">"):
            if name is not None:
                out[name] = b"".join(parts)
            words = line[1:].split()
            name, parts = (words[0] if words else b""), []
        elif name is not None:
            parts.append(line.strip())
    if name is not None:
        out[name] = b"".join(parts)
    return out


# ---- the BLAST table ------------------------------------------------------------------------------------------------------------------

def table_lines(text: bytes):
    """cut at LF, a last line without LF is a line (what palace_sam_lines cuts)"""
    if not text:
        return []
    lines = text.split(b"\n")
    return lines[:-1] if text.endswith(b"\n") else lines


def blast_line(line: bytes):
    """-> ("L", identity digits as an integer, decimals, length) or ("E", code): the checks in csrc/blast_line.hpp's order"""
    t = line.split(b"\t")
    if len(t) < 4:
        return ("E", E_COLUMNS)
    if t[0] == b"" or t[1] == b"":
        return ("E", E_NAME)
    if not _IDENTITY.match(t[2]):
        return ("E", E_IDENTITY)
    if not _LENGTH.match(t[3]):
        return ("E", E_LENGTH)
    whole, _, frac = t[2].partition(b".")
    return ("L", int(whole + frac), len(frac), int(t[3]))


def dump_blast(text: bytes):
    """what `blast_line_selftest lines` prints"""
    return [b"E %d" % r[1] if r[0] == "E" else b"L %d %d %d" % r[1:] for r in map(blast_line, table_lines(text))]


def identity_cuts(threshold: float):
    """cut[k]: the smallest integer N in [0, 10^(3 + k)] with N / 10^k > threshold as doubles (bisection: the quotient does not fall)"""
    cuts = []
    for k in range(7):
        lo, hi = 0, 10 ** (3 + k)
        while lo < hi:
            mid = (lo + hi) // 2
            if float(mid) / float(10 ** k) > threshold:
                hi = mid
            else:
                lo = mid + 1
        cuts.append(lo)
    return cuts


def blast_groups(text: bytes, lengths: dict, ratio: float, cover=None):
    """-> (lines, groups, the flagged names as a set, the first faulty line or 0, its code or 0): the script's loop, line for line, with
    the grammar in front of it; with a fault nothing is flagged"""
    cover = collections.Counter() if cover is None else cover
    lines = table_lines(text)
    prev_key = None
    for no, line in enumerate(lines, 1):
        r = blast_line(line)
        if r[0] == "E":
            return len(lines), 0, set(), no, r[1]
        t = line.split(b"\t")
        if (t[0], t[1]) != prev_key:                      # a group's first line: its query is looked up
            if t[0] not in lengths:
                return len(lines), 0, set(), no, E_QUERY
            if lengths[t[0]] <= 0:
                return len(lines), 0, set(), no, E_QEMPTY
        prev_key = (t[0], t[1])
    blast_segs, groups = set(), 0
    prev_seg, prev_ref, prev_len = b"", b"", 0
    for line in lines:
        t = line.strip().split(b"\t")
        if (prev_seg != t[0] and prev_seg != b"") or (prev_ref != t[1] and prev_ref != b""):
            cover["query_with_two_subjects"] += prev_seg == t[0]
            elen = lengths[prev_seg]
            cover["group_at_ratio"] += float(prev_len) / float(elen) == ratio
            if float(prev_len) / float(elen) > ratio:
                blast_segs.add(prev_seg)
                cover["group_flagged"] += 1
            else:
                cover["group_not_flagged"] += 1
            groups += 1
            cover["group_start_passes" if float(t[2]) > ratio * 100 else "group_start_fails"] += 1
            prev_seg, prev_ref, prev_len = t[0], t[1], int(t[3])
        else:
            if prev_seg == b"":
                cover["first_line_passes" if float(t[2]) > ratio * 100 else "first_line_fails"] += 1
            if float(t[2]) > ratio * 100:
                prev_len = prev_len + int(t[3])
                cover["inside_passes"] += 1
            else:
                cover["inside_fails"] += 1
            prev_seg, prev_ref = t[0], t[1]
    if prev_seg != b"":
        elen = lengths[prev_seg]
        cover["group_at_ratio"] += float(prev_len) / float(elen) == ratio
        if float(prev_len) / float(elen) > ratio:
            blast_segs.add(prev_seg)
            cover["group_flagged"] += 1
        else:
            cover["group_not_flagged"] += 1
        groups += 1
    else:
        cover["empty_table"] += 1
    return len(lines), groups, blast_segs, 0, 0


# ---- scores, hits, paths ----------------------------------------------------------------------------------------------------------------

def read_scores(text: bytes, cover=None):
    cover = collections.Counter() if cover is None else cover
    phagescore = {}
    for no, s in enumerate(file_lines(text), 1):
        item = s.strip().split(b"\t")
        if len(item) != 2 or item[0] == b"":
            raise Fault("scores", no, b"not two columns")
        if not _NUMBER.match(item[1]):
            raise Fault("scores", no, b"a score that is not a decimal number")
        if float(item[1]) >= 0.7:
            if item[0] in phagescore:
                cover["score_replaced_lower" if float(item[1]) < phagescore[item[0]] else "score_replaced"] += 1
            phagescore[item[0]] = float(item[1])
            cover["score_%s" % item[1].decode()] += 1
        else:
            cover["score_below" if item[0] not in phagescore else "score_lower_second_ignored"] += 1
            cover["score_%s" % item[1].decode()] += 1
    return phagescore


def read_hits(text: bytes):
    genehit = []
    for s in file_lines(text):
        item = s.strip().split(b"\t")
        if len(s.strip()) == 0:
            continue
        genehit.append(item[0])
    return genehit


def token_fault(tok: bytes):
    if len(tok) < 2 or tok[-1:] not in (b"+", b"-") or any(c in tok[:-1] for c in (b"+", b"-", b" ")):
        return b"token '" + tok + b"' is not a name followed by + or -"
    if any(w in tok[:-1] for w in RESERVED):
        return b"name '" + tok[:-1] + b"' holds one of ref, self, gene, score, cycle"
    return None


def check_paths(paths: bytes, lengths: dict):
    """the strict grammar of the paths file: the smallest faulty line"""
    for no, line in enumerate(file_lines(paths), 1):
        if line.startswith(b"iter") or line.startswith(b"self") or line.strip() == b"":
            continue
        toks = line.strip().split(b"\t")
        for t in toks:
            why = token_fault(t)
            if why:
                raise Fault("paths", no, why)
        for t in toks:
            if t[:-1] not in lengths:
                raise Fault("paths", no, b"name '" + t[:-1] + b"' is no record of the FASTA")


def path_class(n_tok, tag, gene, s07, s09, all_len, blast_len):
    """the class byte of a path from its facts (include/palace_hip.h: palace_filter_result_plan)"""
    if n_tok == 1 and tag & TAG_SELF:
        return SELFGENE if gene or s07 else WRITE | PLAIN
    if n_tok == 0:
        return 0
    out = 0
    if tag & TAG_CYCLE:
        out |= (CYCLEGENE if gene else 0) | (CYCLESCORE if s09 else 0)
    flags = gene or (all_len != 0 and float(blast_len) / float(all_len) > 0.2)
    if not flags and (not s09 or all_len < 1000):
        return out
    return out | WRITE | (GENESCORE if gene and s09 else 0)


Result = collections.namedtuple("Result", "fasta said cycle classes tags joined all_len cover")


def filter_result(fasta: bytes, paths: bytes, blast: bytes, ratio_text: bytes, hits: bytes, scores: bytes):
    """the command.  Raises Fault(which, line, reason) in the order the executable looks: blast, scores, paths"""
    cover = collections.Counter()
    blast_ratio = float(ratio_text)
    records = parse_fasta(fasta)
    fai_len = {k: len(v) for k, v in records.items()}
    _, _, blast_segs, bad_line, bad_code = blast_groups(blast, fai_len, blast_ratio, cover)
    if bad_line:
        raise Fault("blast", bad_line, BLAST_REASON[bad_code])
    phagescore = read_scores(scores, cover)
    genehit = read_hits(hits)
    check_paths(paths, fai_len)

    def contains_gen(tmp):
        return any(t[:-1] in genehit for t in tmp)

    def max_score(tmp):
        return max([phagescore[t[:-1]] for t in tmp if t[:-1] in phagescore] + [0])

    def sequence(tmp):
        return b"".join(records[t[:-1]] if t[-1:] == b"+" else records[t[:-1]].translate(_COMP)[::-1] for t in tmp)

    out, said, in_faout, res_count = [], [], set(), {}
    classes, tags, joined_of, all_lens = [], [], [], []

    def write(tmp):
        cover["write_first" if b"".join(tmp) not in in_faout else "write_again"] += 1
        if b"".join(tmp) not in in_faout:
            out.append(b">" + b"".join(tmp) + b"\n" + sequence(tmp) + b"\n")
            in_faout.add(b"".join(tmp))

    self_tag = cycle_tag = False
    seen_path = False
    for line in file_lines(paths):
        if line.startswith(b"iter") or line.startswith(b"self"):
            cover["header_after_paths" if seen_path else "header_before_paths"] += 1
            if line.startswith(b"self"):
                self_tag = True
            if line.startswith(b"iter"):
                cycle_tag = True
            continue
        if line.strip() == b"":
            cover["blank_line"] += 1
            continue
        seen_path = True
        tmp = line.strip().split(b"\t")
        joined = b"".join(tmp)
        cls = 0
        cover["path_tags_%d%d" % (self_tag, cycle_tag)] += 1
        all_len = sum(fai_len[t[:-1]] for t in tmp)
        joined_of.append(joined)
        all_lens.append(all_len)
        tags.append((TAG_SELF if self_tag else 0) | (TAG_CYCLE if cycle_tag else 0))
        if len(tmp) == 1 and self_tag:
            cover["single_self_under_cycle" if cycle_tag else "single_self"] += 1
            if contains_gen(tmp) or max_score(tmp) > 0.7:
                cover["selfgene_by_gene" if contains_gen(tmp) else "selfgene_by_score"] += 1
                said.append(b"selfgene" + joined)
                res_count.setdefault(b"selfgene" + joined)
                cls |= SELFGENE
            else:
                cover["self_plain"] += 1
                write(tmp)
                res_count.setdefault(joined)
                cls |= WRITE | PLAIN
            classes.append(cls)
            continue
        if self_tag:
            cover["multi_token_under_self"] += 1
        if len(tmp) == 1:
            cover["single_token_not_self"] += 1
        if cycle_tag:
            cover["cycle_gene" if contains_gen(tmp) else "cycle_no_gene"] += 1
            if contains_gen(tmp):
                said.append(b"cyclegene" + joined)
                res_count.setdefault(b"cyclegene" + joined)
                cls |= CYCLEGENE
            cover["cycle_score" if max_score(tmp) >= 0.9 else "cycle_no_score"] += 1
            if max_score(tmp) >= 0.9:
                said.append(b"cyclescore" + joined)
                res_count.setdefault(b"cyclescore" + joined)
                cls |= CYCLESCORE
        flags = False
        blast_len = 0
        if contains_gen(tmp):
            flags = True
        blast_len = sum(fai_len[t[:-1]] for t in tmp if t[:-1] in blast_segs)
        if all_len != 0:
            cover["blast_share_at_0.2"] += float(blast_len) / float(all_len) == 0.2
        if all_len != 0 and (float(blast_len) / float(all_len)) > 0.2:
            flags = True
            cover["flags_by_blast"] += 1
        if all_len in (999, 1000, 9999, 10000):
            cover["all_len_%d" % all_len] += 1
        if not flags and (max_score(tmp) < 0.9 or all_len < 1000):
            cover["dropped_no_score" if max_score(tmp) < 0.9 else "dropped_short"] += 1
            classes.append(cls)
            continue
        cover["kept_by_flags" if flags else "kept_by_score_and_length"] += 1
        cls |= WRITE
        if contains_gen(tmp) and max_score(tmp) >= 0.9:
            said.append(b"genescore" + joined)
            cls |= GENESCORE
            write(tmp)
        else:
            if max_score(tmp) >= 0.9:
                write(tmp)
            elif contains_gen(tmp):
                write(tmp)
            if flags:
                write(tmp)
        classes.append(cls)

    cycle = []
    for s in res_count:                                   # OUR order: first appearance (the reference's is a set's)
        sresult = s.replace(b"self", b"").replace(b"gene", b"").replace(b"score", b"")
        s_len = sum(fai_len[v.replace(b"cycle", b"")] for v in re.split(rb"[+-]", sresult) if v != b"")
        cover["cycle_line" if s_len >= 10000 else "cycle_short"] += 1
        if s_len >= 10000:
            cycle.append(sresult)
    return Result(b"".join(out), said, cycle, classes, tags, joined_of, all_lens, cover)


def first_of_equal(codes, classes):
    """codes[p]: a path's code sequence (a tuple), classes[p] its class byte -> per path the bits for which it is the first path, in
    order, with that bit among the paths with an identical sequence"""
    seen, out = set(), []
    for seq, cls in zip(codes, classes):
        v = 0
        for c in range(6):
            if cls >> c & 1 and (seq, c) not in seen:
                seen.add((seq, c))
                v |= 1 << c
        out.append(v)
    return out


def outputs_from_classes(res: Result):
    """the three outputs' skeleton from classes and first_of_equal, as the executable derives them: (headers written, stdout, cycle)"""
    first = first_of_equal([(j,) for j in res.joined], res.classes)
    said, cycle, written = [], [], []
    for j, cls, f, n in zip(res.joined, res.classes, first, res.all_len):
        said += [w + j for w, bit in zip(TAGGED, (SELFGENE, CYCLEGENE, CYCLESCORE, GENESCORE)) if cls & bit]
        if n >= 10000:
            cycle += [(b"cycle" if bit >= CYCLEGENE else b"") + j for bit in (PLAIN, SELFGENE, CYCLEGENE, CYCLESCORE) if f & bit]
        if f & WRITE:
            written.append(j)
    return written, said, cycle


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------

def make_sequence(rng, length):
    """a sequence with a short period (it compresses), ambiguity codes and lower case among it"""
    motif = bytes(rng.choice(list(b"ACGTACGTACGTRYKMBDHVNacgtn"), size=int(rng.integers(5, 14))).astype(np.uint8))
    return (motif * (length // len(motif) + 1))[:length]


def make_fasta(rng, specs, width=0):
    out = []
    for k, (name, length) in enumerate(specs):
        seq = make_sequence(rng, length)
        out.append(b">" + name + (b" note %d" % k if k % 3 == 0 else b"") + b"\n")
        if width:
            out += [seq[i:i + width] + b"\n" for i in range(0, len(seq), width)]
        else:
            out.append(seq + b"\n")
    return b"".join(out)


def _edges(ratio_text):
    rng = np.random.default_rng(5)
    specs = [(b"a1", 1), (b"a4", 4), (b"e1", 1), (b"c100", 100), (b"t10", 10), (b"u10", 10), (b"v10", 10), (b"d949", 949), (b"d950", 950), (b"k9999", 9999),
             (b"k10000", 10000), (b"g50", 50), (b"s70", 50), (b"s71", 50), (b"s90", 50), (b"s89", 50), (b"x20", 20), (b"y20", 20), (b"dd", 30), (b"de", 30),
             (b"NODE_7_length_12_cov_1.5", 12)]
    fasta = make_fasta(rng, specs, 60)
    blast = b"".join(b"\t".join(r) + b"\t0\t0\t1\t2\t3\t4\t1e-5\t50\n" for r in [
        (b"a1", b"S0", b"50.0", b"1"),                     # the table's first line fails the identity: nothing in its sum
        (b"c100", b"S1", b"80.0", b"50"), (b"c100", b"S1", b"90", b"25"), (b"c100", b"S1", b"60.5", b"10"),      # 75 / 100
        (b"c100", b"S2", b"10.0", b"76"),                  # a group's first line below the identity, counted all the same: 76 / 100
        (b"t10", b"S1", b"20", b"7"),                      # 7 / 10
        (b"u10", b"S1", b"20", b"7"), (b"u10", b"S1", b"75.0", b"1"), (b"u10", b"S1", b"75", b"1"), (b"u10", b"S1", b"75.000000", b"1"),
        (b"v10", b"S1", b"1", b"7"), (b"v10", b"S1", b"75.000001", b"1"), (b"v10", b"S1", b"70.000000", b"5"), (b"v10", b"S1", b"70.000001", b"0"),
        (b"e1", b"S9", b"99.999999", b"1"),
        (b"NODE_7_length_12_cov_1.5", b"S1", b"100", b"0000000009")])
    hits = b"g50\tPF001\t1e-9\n\n  \nnot_in_the_assembly\tx\ng50\n"
    scores = (b"s70\t0.7\ns71\t0.70000001\ns90\t0.9\ns89\t0.8999\nx20\t0.6999\ndd\t0.95\ndd\t0.5\nde\t0.95\nde\t0.8\nnot_in_the_assembly\t0.99\n"
              b"y20\t1e-1\n")
    paths = b"".join(b"\t".join(p) + b"\n" for p in [
        (b"x20+", b"y20-"), (b"e1+", b"a4-"), (b"e1+", b"a1+"), (b"g50+", b"x20+"), (b"s90+", b"d950+"), (b"s90+", b"d949+"), (b"s89+", b"d950+"),
        (b"g50+", b"s90-"), (b"x20+",), (b"c100+",), (b"t10-",), (b"u10-",), (b"v10-",)])
    paths += b"self loops\n" + b"".join(b"\t".join(p) + b"\n" for p in [
        (b"x20+",), (b"c100+",), (b"g50+",), (b"s71-",), (b"s70+",), (b"x20+", b"y20-"), (b"g50+", b"x20+"), (b"k10000+",), (b"k9999-",), (b"dd+",), (b"de-",),
        (b"x20-",), (b"k10000+", b"g50-")])
    paths += b"\n   \t \n" + b"iter 1\n" + b"".join(b"\t".join(p) + b"\n" for p in [
        (b"g50+", b"k10000-"), (b"s90+", b"k10000-"), (b"g50+", b"s90-", b"k10000+"), (b"g50+", b"k10000-"), (b"x20+",), (b"k10000+",), (b"dd+", b"d950+"),
        (b"de+", b"d950+"), (b"s90+", b"k9999+"), (b"g50+", b"k9999+"), (b"s90+", b"d949+", b"NODE_7_length_12_cov_1.5-"), (b"x20+", b"y20-"), (b"g50+",)])
    paths += b"self again\n" + b" k9999+\t\n" + b"iter 2\n" + b"s90-\tk10000+\tx20+"          # (no LF at the end)
    return fasta, paths, blast, ratio_text, hits, scores


def _headers_first():
    """both headers in front of every path, `iter` first; a one-line table whose line passes"""
    rng = np.random.default_rng(6)
    fasta = make_fasta(rng, [(b"p%d" % k, n) for k, n in enumerate((40, 60, 10000, 5, 700, 300))])
    blast = b"p0\tS\t99.1\t39\textra"
    paths = b"iter 0\nself\np0+\np1-\np0+\tp1-\np2+\np2+\tp3-\np4+\tp5+\np4+\tp5+\n"
    return fasta, paths, blast, b"0.75", b"p3\n", b"p4\t0.9\np1\t0.71\n"


def _cycle_only():
    """`iter` without `self`: one-token lines are ordinary lines"""
    rng = np.random.default_rng(7)
    fasta = make_fasta(rng, [(b"q%d" % k, n) for k, n in enumerate((10000, 9999, 1, 1000, 999, 50))], 70)
    blast = b"q5\tS\t80\t10\nq5\tS\t80\t10\nq5\tT\t80\t45\nq3\tT\t100\t751\n"
    paths = b"q0+\nq5+\niter 1\nq0+\nq0-\nq1+\nq2+\tq1-\nq3+\nq4+\nq5+\nq5+\tq0+\nq3-\tq0+\nq4+\tq2+\n"
    return fasta, paths, blast, b"0.75", b"q0\nq2\tx\n", b"q0\t0.9\nq1\t1\nq4\t0.95\n"


def _random(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(12, 40))
    lens = [int(rng.choice([1, 4, 5, 20, 100, 250, 400, 999, 1000])) for _ in range(n)]
    if seed % 3 == 0:
        lens[0], lens[1] = 6000, 4000
    names = [b"EDGE_%d_length_%d_cov_%d.%d" % (k + 1, L, rng.integers(1, 90), rng.integers(0, 10)) for k, L in enumerate(lens)]
    fasta = make_fasta(rng, list(zip(names, lens)), int(rng.choice([0, 60, 80])))
    ratio_text = [b"0.75", b"0.7", b"0.5"][seed % 3]
    rows = []
    for _ in range(int(rng.integers(0, 25))):
        q, s = int(rng.integers(0, n)), b"REF%d" % rng.integers(0, 3)
        for _ in range(int(rng.integers(1, 5))):
            ident = [b"%d" % rng.integers(40, 101), b"%d.%d" % (rng.integers(40, 100), rng.integers(0, 1000)), b"75.0", b"70.000", b"50.000001"][int(rng.integers(0, 5))]
            rows.append(b"%s\t%s\t%s\t%d\t0\t0\n" % (names[q], s, ident, rng.integers(0, lens[q] + 1)))
    blast = b"".join(rows)
    if seed % 4 == 1 and blast:
        blast = blast[:-1]
    hits = b"".join(b"%s\tfam%d\n" % (names[int(k)], k) for k in rng.integers(0, n, size=int(rng.integers(0, 6))))
    values = [b"0.7", b"0.70000001", b"0.9", b"0.8999", b"0.95", b"0.3", b"1.0", b"0.75"]
    scores = b"".join(b"%s\t%s\n" % (names[int(k)], values[int(rng.integers(0, len(values)))]) for k in rng.integers(0, n, size=int(rng.integers(0, 14))))
    lines = []
    for _ in range(int(rng.integers(5, 45))):
        u = rng.random()
        if u < 0.06:
            lines.append(b"self_loop:\n")
        elif u < 0.12:
            lines.append(b"iter %d\n" % rng.integers(0, 9))
        elif u < 0.16:
            lines.append(b"\n")
        elif u < 0.30 and lines:
            lines.append(lines[int(rng.integers(0, len(lines)))])
        else:
            k = int(rng.choice([1, 1, 2, 2, 3, 5, 9]))
            lines.append(b"\t".join(names[int(t)] + (b"+", b"-")[int(rng.integers(0, 2))] for t in rng.integers(0, n, size=k)) + b"\n")
    return fasta, b"".join(lines), blast, ratio_text, hits, scores


def golden_inputs():
    cases = {"edges_075": _edges(b"0.75"), "edges_07": _edges(b"0.7"), "headers_first": _headers_first(), "cycle_only": _cycle_only()}
    f, p, b, r, h, s = cases["edges_075"]
    cases["empty_blast"] = (f, p, b"", r, h, s)
    cases["empty_hits_and_scores"] = (f, p, b, r, b"", b"")
    cases["empty_paths"] = (f, b"", b, r, h, s)
    for seed in range(1, 17):
        cases["random_%d" % seed] = _random(seed)
    return cases


def faulty_inputs():
    """name -> (which, (fasta, paths, blast, ratio, hits, scores), line, reason): one file outside the grammar, the others a golden case's"""
    f, p, b, r, h, s = golden_inputs()["headers_first"]
    out = {}
    for name, text, line, code in (("blast_three_columns", b"p0\tS\t99\t1\np0\tS\t99\n", 2, E_COLUMNS), ("blast_blank_line", b"p0\tS\t99\t1\n\np0\tS\t99\t1\n", 2, E_COLUMNS),
                                   ("blast_empty_subject", b"p0\t\t99\t1\n", 1, E_NAME), ("blast_exponent", b"p0\tS\t99\t1\np0\tS\t1e2\t1\n", 2, E_IDENTITY),
                                   ("blast_signed_length", b"p0\tS\t99\t+5\n", 1, E_LENGTH), ("blast_unknown_query", b"p0\tS\t99\t1\nzz\tS\t99\t1\nzz\tS\tx\t1\n", 2, E_QUERY),
                                   ("blast_two_faults", b"p0\tS\t99\t1\np1\tS\t99.\t1\np0\tS\n", 2, E_IDENTITY)):
        out[name] = ("blast", (f, p, text, r, h, s), line, BLAST_REASON[code])
    out["blast_empty_record"] = ("blast", (f + b">hollow\n", p, b"p0\tS\t99\t1\nhollow\tS\t99\t1\n", r, h, s), 2, BLAST_REASON[E_QEMPTY])
    out["scores_one_column"] = ("scores", (f, p, b, r, h, b"p4\t0.9\n\np1\t0.8\n"), 2, b"not two columns")
    out["scores_not_a_number"] = ("scores", (f, p, b, r, h, b"p4\t0.9\np1\t+0.8\np1\tx\n"), 2, b"a score that is not a decimal number")
    out["paths_no_strand"] = ("paths", (f, b"p0+\np1\n", b, r, h, s), 2, b"token 'p1' is not a name followed by + or -")
    out["paths_empty_token"] = ("paths", (f, b"p0+\t\tp1-\n", b, r, h, s), 1, b"token '' is not a name followed by + or -")
    out["paths_space"] = ("paths", (f, b"self\np0+ p1-\n", b, r, h, s), 2, b"token 'p0+ p1-' is not a name followed by + or -")
    out["paths_reserved_word"] = ("paths", (f + b">myscore1\nAC\n", b"p0+\nmyscore1+\n", b, r, h, s), 2, b"name 'myscore1' holds one of ref, self, gene, score, cycle")
    out["paths_unknown_name"] = ("paths", (f, b"p0+\nzz+\tp1-\np1\n", b, r, h, s), 2, b"name 'zz' is no record of the FASTA")
    out["paths_second_try_is_not_found"] = ("paths", (f, b"p0_7+\n", b, r, h, s), 1, b"name 'p0_7' is no record of the FASTA")
    return out


def malformed_tables():
    """tables for the line reader alone: the catalogue's, cut and bent"""
    out = [b"", b"\n", b"a\tb\t1\t2", b"a\tb\t1\t2\n\n", b"a\tb\t100.000000\t1234567890\tx\n", b"a\tb\t1000\t1\n", b"a\tb\t1.0000000\t1\n", b"a\tb\t.5\t1\n",
           b"a\tb\t5.\t1\n", b"a\tb\t-5\t1\n", b"a\tb\t5\t12345678901\n", b"a\tb\t5\t\n", b"a\tb\t5\t1 \n", b"a\tb\t5\t1\r\n", b"a\tb\t5\t1\tz\r\n", b"\tb\t5\t1\n",
           b"a\t\t5\t1\n", b"a\tb\t\t1\n", b"\t\t\t\n", b"a b\tc\t 5\t1\n", b"a\tb\t5e1\t1\n", b"a\tb\t5\t1e1\n", b"a\tb\t5.5.5\t1\n", b"x" * 300 + b"\ty\t9\t9\n"]
    for case in golden_inputs().values():
        table = case[2]
        out.append(table)
        out.append(table.replace(b"\t", b" ", 3))
        out.append(table.replace(b".", b",", 2))
        out.append(table[:len(table) // 2])
    return out


def hand_checks():
    fasta = b">a x\nACGTR\n>b\nAAAAACCCCC\n"
    # the first line is inside its group: 50 fails, so a's sum is 0 + nothing; b: the group start counts though 10 < 75, then 3 more
    res = filter_result(fasta, b"a+\tb-\nself\na-\nb+\n", b"a\tS\t50\t5\nb\tS\t10\t5\nb\tS\t80\t3\n", b"0.75", b"", b"b\t0.8\n")
    assert blast_groups(b"a\tS\t50\t5\nb\tS\t10\t5\nb\tS\t80\t3\n", {b"a": 5, b"b": 10}, 0.75)[:3] == (3, 2, {b"b"})
    assert res.fasta == b">a+b-\nACGTRGGGGGTTTTT\n>a-\nYACGT\n" and res.said == [b"selfgeneb+"] and res.cycle == []
    assert res.classes == [WRITE, WRITE | PLAIN, SELFGENE]
    assert blast_groups(b"a\tS\t50\t5\nb\tS\t10\t5\nb\tS\t80\t3\n", {b"a": 5, b"b": 10}, 0.8)[2] == set()          # 8 / 10 is not > 0.8
    assert blast_groups(b"a\tS\t76\t4\n", {b"a": 5}, 0.75)[2] == {b"a"} and blast_groups(b"a\tS\t75.0\t5\n", {b"a": 5}, 0.75)[2] == set()
    assert blast_line(b"a\tb\t99.50\t12\tx") == ("L", 9950, 2, 12) and blast_line(b"a\tb\t99.\t12") == ("E", E_IDENTITY)
    assert identity_cuts(75.0) == [76, 751, 7501, 75001, 750001, 7500001, 75000001] and identity_cuts(0.29 * 100)[0] == 29
    assert first_of_equal([(1,), (1,), (2,), (1,)], [SELFGENE, WRITE | PLAIN, WRITE, WRITE | SELFGENE]) == [SELFGENE, WRITE | PLAIN, WRITE, 0]
    for name, case in golden_inputs().items():
        res = filter_result(*case)
        written, said, cycle = outputs_from_classes(res)
        assert said == res.said and cycle == res.cycle and written == [rec.split(b"\n")[0] for rec in res.fasta.split(b">")[1:]], name
    for name, (which, case, line, reason) in faulty_inputs().items():
        try:
            filter_result(*case)
            raise AssertionError(name)
        except Fault as e:
            assert (e.which, e.line, e.reason) == (which, line, reason), (name, e.which, e.line, e.reason)


if __name__ == "__main__":
    hand_checks()
    total = collections.Counter()
    for case in golden_inputs().values():
        total += filter_result(*case).cover
    print(len(golden_inputs()), "cases;", dict(sorted(total.items())))
