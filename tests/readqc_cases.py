"""The rules of `readqc` restated in Python, written from the rules and not from csrc/fastq_rules.hpp: the grammar verdict
of a FASTQ text, the overlap search of a pair, the trim, the filter, the two output texts and the report's counts; and the builders
of the cases the tests share.  fastp is absent: these rules are the behaviour (parity unpinned)."""
import numpy as np

ELINES, EAT, EPLUS, ELONG, EBASE, EQLEN, EQUAL, ECOUNT = range(1, 9)     # PALACE_FASTQ_E* of include/palace_hip.h
MAX_SEQ = 4096
PASS, LOW_QUALITY, TOO_MANY_N, TOO_SHORT = range(4)
DEFAULTS = dict(qualified_quality=15, unqualified_percent=40, n_limit=5, min_length=15, no_trim=0, no_quality_filter=0, no_length_filter=0,
                overlap_require=30, diff_limit=5, diff_pct=20, diff_window=50)
COUNTS = ("reads_before", "bases_before", "reads_after", "bases_after", "low_quality", "too_many_n", "too_short", "trimmed_reads", "trimmed_bases")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def params(**kw):
    p = dict(DEFAULTS)
    assert set(kw) <= set(p), kw
    p.update(kw)
    return p


# ---- the grammar -----------------------------------------------------------------------------------------------------------------------
def lines_of(text: bytes):
    """cut at LF; a last line without LF is a line; the empty text has no line"""
    if not text:
        return []
    lines = text.split(b"\n")
    if text.endswith(b"\n"):
        lines.pop()
    return lines


def verdict(text: bytes):
    """(complete records, the smallest faulty line 1-based, its code), 0 / 0 for a valid text"""
    lines = lines_of(text)
    n = len(lines) // 4
    for r in range(n):
        name, seq, plus, qual = lines[4 * r:4 * r + 4]
        if not name.startswith(b"@"):
            return n, 4 * r + 1, EAT
        if len(seq) > MAX_SEQ:
            return n, 4 * r + 2, ELONG
        if any(c not in b"ACGTN" for c in seq):
            return n, 4 * r + 2, EBASE
        if not plus.startswith(b"+"):
            return n, 4 * r + 3, EPLUS
        if len(qual) != len(seq):
            return n, 4 * r + 4, EQLEN
        if any(not 33 <= c <= 126 for c in qual):
            return n, 4 * r + 4, EQUAL
    if len(lines) % 4:
        return n, 4 * n + 1, ELINES
    return n, 0, 0


def records_of(text: bytes):
    lines = lines_of(text)
    return [tuple(lines[4 * r:4 * r + 4]) for r in range(len(lines) // 4)]


# ---- the overlap -----------------------------------------------------------------------------------------------------------------------
def revcomp(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def candidates(l1: int, l2: int, p):
    req = p["overlap_require"]
    return [(o, 0, min(l1 - o, l2)) for o in range(max(0, l1 - req))] + [(0, k, min(l1, l2 - k)) for k in range(max(0, l2 - req))]


def accepted(a: bytes, b: bytes, cand, p) -> bool:
    a0, b0, n = cand
    limit = min(p["diff_limit"], n * p["diff_pct"] // 100)
    m = min(n, p["diff_window"])
    diff = 0
    for x, y in zip(a[a0:a0 + m], b[b0:b0 + m]):
        if x != y:
            diff += 1
            if diff > limit:                                                # (over the limit it stays over it: the count's end changes nothing)
                return False
    return True


def overlap(seq1: bytes, seq2: bytes, p=DEFAULTS):
    """(index of the first accepted candidate in search order or -1, that candidate or None)"""
    a, b = seq1, revcomp(seq2)
    for c, cand in enumerate(candidates(len(a), len(b), p)):
        if accepted(a, b, cand, p):
            return c, cand
    return -1, None


def literal_overlap(seq1: bytes, seq2: bytes, p=DEFAULTS):
    """the loop the "first 50" form was derived from: it counts over all n positions, breaks when the count exceeds the limit at i < 50,
    and accepts when the count is <= limit, or when it is over the limit and the walk ended at i > 50.  -> (offset, n) with a negative
    offset for a reverse hit (-k), or None"""
    a, b = seq1, revcomp(seq2)
    l1, l2, req, win = len(a), len(b), p["overlap_require"], p["diff_window"]

    def walk(a0, b0, n):
        limit = min(p["diff_limit"], n * p["diff_pct"] // 100)
        diff, i = 0, 0
        while i < n:
            if a[a0 + i] != b[b0 + i]:
                diff += 1
                if diff > limit and i < win:
                    break
            i += 1
        return diff <= limit or (diff > limit and i > win)
    o = 0
    while o < l1 - req:
        n = min(l1 - o, l2)
        if walk(o, 0, n):
            return o, n
        o += 1
    k = 0
    while k < l2 - req:
        n = min(l1, l2 - k)
        if walk(0, k, n):
            return -k, n
        k += 1
    return None


def trim_to(seq1: bytes, seq2: bytes, p=DEFAULTS):
    """the bases both reads keep, or None where nothing is trimmed: only a first accepted candidate that is a reverse one with k >= 1 trims"""
    if p["no_trim"]:
        return None
    _, cand = overlap(seq1, seq2, p)
    if cand is None or cand[1] < 1:
        return None
    return cand[2]


# ---- the filter ------------------------------------------------------------------------------------------------------------------------
def read_filter(seq: bytes, qual: bytes, p=DEFAULTS) -> int:
    ln = len(seq)
    if not p["no_quality_filter"]:
        low = sum(1 for c in qual if c < 33 + p["qualified_quality"])
        if low * 100 > p["unqualified_percent"] * ln:
            return LOW_QUALITY
        if seq.count(b"N") > p["n_limit"]:
            return TOO_MANY_N
    if not p["no_length_filter"] and ln < p["min_length"]:
        return TOO_SHORT
    return PASS


def run_pair(rec1, rec2, p=DEFAULTS):
    """-> (bases read 1 keeps, read 2 keeps, the pair's reason: PASS or why it is dropped)"""
    n = trim_to(rec1[1], rec2[1], p)
    k1 = len(rec1[1]) if n is None else min(n, len(rec1[1]))
    k2 = len(rec2[1]) if n is None else min(n, len(rec2[1]))
    r1, r2 = read_filter(rec1[1][:k1], rec1[3][:k1], p), read_filter(rec2[1][:k2], rec2[3][:k2], p)
    return k1, k2, r1 or r2


def readqc(text1: bytes, text2: bytes, p=DEFAULTS):
    """two valid texts of equal record counts -> dict: out1, out2 (the output texts), len1, len2 (kept bases or -1), off1, off2, and COUNTS"""
    recs1, recs2 = records_of(text1), records_of(text2)
    assert len(recs1) == len(recs2)
    res = {k: 0 for k in COUNTS}
    out, lens, offs = ([], []), ([], []), ([0], [0])
    for a, b in zip(recs1, recs2):
        k1, k2, reason = run_pair(a, b, p)
        res["reads_before"] += 2
        res["bases_before"] += len(a[1]) + len(b[1])
        res["trimmed_reads"] += (k1 < len(a[1])) + (k2 < len(b[1]))
        res["trimmed_bases"] += len(a[1]) - k1 + len(b[1]) - k2
        if reason:
            res[("low_quality", "too_many_n", "too_short")[reason - 1]] += 2
        else:
            res["reads_after"] += 2
            res["bases_after"] += k1 + k2
        for w, (rec, k) in enumerate(((a, k1), (b, k2))):
            text = b"" if reason else rec[0] + b"\n" + rec[1][:k] + b"\n" + rec[2] + b"\n" + rec[3][:k] + b"\n"
            out[w].append(text)
            lens[w].append(-1 if reason else k)
            offs[w].append(offs[w][-1] + len(text))
    res.update(out1=b"".join(out[0]), out2=b"".join(out[1]), len1=np.array(lens[0], np.int32), len2=np.array(lens[1], np.int32),
               off1=np.array(offs[0], np.int64), off2=np.array(offs[1], np.int64))
    return res


def report(res):
    """the JSON of -j as a dict"""
    return {"summary": {"before_filtering": {"total_reads": res["reads_before"], "total_bases": res["bases_before"]},
                        "after_filtering": {"total_reads": res["reads_after"], "total_bases": res["bases_after"]}},
            "filtering_result": {"passed_filter_reads": res["reads_after"], "low_quality_reads": res["low_quality"],
                                 "too_many_N_reads": res["too_many_n"], "too_short_reads": res["too_short"]},
            "adapter_cutting": {"adapter_trimmed_reads": res["trimmed_reads"], "adapter_trimmed_bases": res["trimmed_bases"]}}


# ---- the case builders -----------------------------------------------------------------------------------------------------------------
def random_seq(rng, n: int) -> bytes:
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)])


def other_base(c: int) -> int:
    return b"CGTA"[b"ACGT".index(c)] if c in b"ACGT" else ord("A")


def pair_with_insert(rng, l1: int, l2: int, insert: int, mismatches_at=(), frag=None):
    """(seq1, seq2) of a fragment of `insert` bases (random, or `frag`): read 1 is its first l1 bases, read 2 the reverse complement of
    its last l2, each running into a random adapter-like tail where the fragment is shorter than the read.  mismatches_at: positions of
    the fragment (counted from its start) changed in read 1 only.  With insert < l2 the reverse candidate k = l2 - insert overlaps
    n = min(l1, insert); with insert >= l2 the forward candidate o = insert - l2 overlaps l1 - o."""
    frag = random_seq(rng, insert) if frag is None else frag
    assert len(frag) == insert
    one = bytearray((frag + random_seq(rng, max(0, l1 - insert)))[:l1])
    two = (revcomp(frag) + random_seq(rng, max(0, l2 - insert)))[:l2]
    for at in mismatches_at:
        if at < len(one):
            one[at] = other_base(one[at])
    return bytes(one), two


def qual_with_low(rng, ln: int, low: int, threshold: int = 15) -> bytes:
    """ln QUAL bytes of which exactly `low` lie below 33 + threshold, at random places"""
    q = np.full(ln, 33 + threshold + 10, np.uint8)
    q[rng.permutation(ln)[:low]] = 33 + threshold - 1
    return q.tobytes()


def fastq(records, last_lf: bool = True) -> bytes:
    """records of (name without '@', seq, qual) or (name, seq, qual, plus line)"""
    text = b"".join(b"@" + r[0] + b"\n" + r[1] + b"\n" + (r[3] if len(r) > 3 else b"+") + b"\n" + r[2] + b"\n" for r in records)
    return text if last_lf or not text else text[:-1]


def random_pairs(rng, n: int, lengths=(0, 1, 14, 15, 16, 29, 30, 31, 32, 49, 50, 51, 52, 64, 65, 100, 150), p_overlap: float = 0.5):
    """n pairs (seq1, qual1, seq2, qual2) over the border lengths: about p_overlap of them sequenced from a fragment shorter than the reads'
    sum (a few mismatches, a few N), the rest unrelated; qualities with a share of low bytes around the filter's border"""
    out = []
    for _ in range(n):
        l1, l2 = (int(rng.choice(lengths)) for _ in range(2))
        if rng.random() < p_overlap and min(l1, l2) > 0:
            insert = int(rng.integers(1, l1 + l2 + 1))
            frag = random_seq(rng, insert)
            one = (frag + random_seq(rng, l1))[:l1]
            two = (revcomp(frag) + random_seq(rng, l2))[:l2]
        else:
            one, two = random_seq(rng, l1), random_seq(rng, l2)
        seqs = []
        for s in (one, two):
            s = bytearray(s)
            for _ in range(int(rng.integers(0, 4)) if rng.random() < 0.5 else 0):
                if s:
                    at = int(rng.integers(0, len(s)))
                    s[at] = other_base(s[at])
            for _ in range(int(rng.integers(0, 9)) if rng.random() < 0.2 else 0):
                if s:
                    s[int(rng.integers(0, len(s)))] = ord("N")
            seqs.append(bytes(s))
        quals = [qual_with_low(rng, len(s), int(rng.integers(0, len(s) + 1)) if rng.random() < 0.3 else min(len(s), len(s) * 2 // 5 + int(rng.integers(-1, 2))) if
                               rng.random() < 0.3 and s else 0) for s in seqs]
        out.append((seqs[0], quals[0], seqs[1], quals[1]))
    return out


def texts_of(pairs, plus=b"+"):
    t1 = fastq([(b"p%d/1" % i, p[0], p[1], plus) for i, p in enumerate(pairs)])
    t2 = fastq([(b"p%d/2 second" % i, p[2], p[3], plus) for i, p in enumerate(pairs)])
    return t1, t2


# ---- the selftest's case file ----------------------------------------------------------------------------------------------------------
def selftest_line(kind: str, *fields) -> bytes:
    """G <hex of a text>     P <flags: letters of AQL or -> <seq1> <qual1> <seq2> <qual2>     (an empty field is written `.`; QUAL as hex)"""
    return (kind + " " + " ".join(f if f else "." for f in fields)).encode() + b"\n"


def selftest_expected(kind: str, *fields) -> bytes:
    if kind == "G":
        return b"G %d %d %d\n" % verdict(bytes.fromhex(fields[0]))
    flags, s1, q1, s2, q2 = fields
    p = params(no_trim="A" in flags, no_quality_filter="Q" in flags, no_length_filter="L" in flags)
    rec1, rec2 = (b"@", s1.encode(), b"+", bytes.fromhex(q1)), (b"@", s2.encode(), b"+", bytes.fromhex(q2))
    c, _ = overlap(rec1[1], rec2[1], p)
    return b"P %d %d %d %d\n" % ((c,) + run_pair(rec1, rec2, p))
