"""What `readqc --full-report` counts (DESIGN.md 8 "Reports"), restated in numpy over readqc_cases' records and overlap search, written
from the rules and not from csrc/fastq_rules.hpp: base slots, QUAL bytes, a pair's insert size, the per-cycle tables of a text and the
report's dict.  fastp is absent: these rules are the behaviour (parity unpinned)."""
import numpy as np

from tests import readqc_cases as rc

SLOTS = b"ACGTN"                  # slot 0 .. 4
ISIZE_MAX = 512                   # PALACE_READQC_ISIZE_MAX: slot 512 is "unknown"
_SLOT_OF = np.full(256, 4, np.int64)
for _k, _c in enumerate(SLOTS):
    _SLOT_OF[_c] = _k


def qual_facts(q: int):
    """a QUAL byte -> (value, counts as Q20, counts as Q30)"""
    return q - 33, q >= 33 + 20, q >= 33 + 30


def insert_size(seq1: bytes, seq2: bytes, p=rc.DEFAULTS):
    """-> (the first accepted candidate's index, -1 for none and under no_trim; the insert size's slot)"""
    if p["no_trim"]:
        return -1, ISIZE_MAX
    c, cand = rc.overlap(seq1, seq2, p)
    if cand is None:
        return -1, ISIZE_MAX
    a0, _, n = cand
    forward = c < max(0, len(seq1) - p["overlap_require"])
    size = len(seq1) + len(seq2) - n if forward and a0 >= 1 else n
    return c, min(size, ISIZE_MAX)


def insert_histogram(text1: bytes, text2: bytes, p=rc.DEFAULTS):
    hist = np.zeros(ISIZE_MAX + 1, np.uint64)
    for a, b in zip(rc.records_of(text1), rc.records_of(text2)):
        hist[insert_size(a[1], b[1], p)[1]] += 1
    return hist


def section(records, lens, max_cycles: int):
    """the tables of the reads' first lens[r] cycles (lens None: all of every read; a negative length: none of it), cycles >= max_cycles
    left out -> dict of cnt, qsum uint64 (max_cycles, 5), q20, q30"""
    seqs, quals = [], []
    for r, rec in enumerate(records):
        k = len(rec[1]) if lens is None else min(max(int(lens[r]), 0), len(rec[1]))
        k = min(k, max_cycles)
        seqs.append(np.frombuffer(rec[1][:k], np.uint8))
        quals.append(np.frombuffer(rec[3][:k], np.uint8))
    cnt, qsum = np.zeros((max_cycles, 5), np.uint64), np.zeros((max_cycles, 5), np.uint64)
    if not seqs or not sum(len(s) for s in seqs):
        return {"cnt": cnt, "qsum": qsum, "q20": 0, "q30": 0}
    cyc = np.concatenate([np.arange(len(s)) for s in seqs])
    slot = _SLOT_OF[np.concatenate(seqs)]
    qual = np.concatenate(quals).astype(np.int64)
    np.add.at(cnt, (cyc, slot), np.uint64(1))
    np.add.at(qsum, (cyc, slot), (qual - 33).astype(np.uint64))
    return {"cnt": cnt, "qsum": qsum, "q20": int(np.sum(qual >= 53)), "q30": int(np.sum(qual >= 63))}


def cycle_stats(text: bytes, lens, max_cycles: int):
    """what palace_readqc_cycle_stats leaves for one text: [before] or, with kept lengths, [before, after]"""
    records = rc.records_of(text)
    return [section(records, None, max_cycles)] + ([] if lens is None else [section(records, lens, max_cycles)])


def same_section(got, want):
    return np.array_equal(got["cnt"], want["cnt"]) and np.array_equal(got["qsum"], want["qsum"]) and (got["q20"], got["q30"]) == (want["q20"], want["q30"])


def _ratio(num: int, den: int) -> float:
    return int(num) / int(den) if den else 0.0


def _read_block(sec, reads: int):
    cnt, qsum = sec["cnt"], sec["qsum"]
    every = cnt.sum(axis=1)
    cycles = int(np.nonzero(every)[0][-1]) + 1 if every.any() else 0         # the longest read of the section
    at = {chr(c): k for k, c in enumerate(SLOTS)}
    quality = {b: [_ratio(qsum[c, at[b]], cnt[c, at[b]]) for c in range(cycles)] for b in "ATCG"}
    quality["mean"] = [_ratio(qsum[c].sum(), every[c]) for c in range(cycles)]
    content = {b: [_ratio(cnt[c, at[b]], every[c]) for c in range(cycles)] for b in "ATCGN"}
    content["GC"] = [_ratio(int(cnt[c, at["G"]]) + int(cnt[c, at["C"]]), every[c]) for c in range(cycles)]
    return {"total_reads": reads, "total_bases": int(every.sum()), "q20_bases": sec["q20"], "q30_bases": sec["q30"], "total_cycles": cycles,
            "quality_curves": quality, "content_curves": content}


def _summary_block(one, two):
    bases = one["total_bases"] + two["total_bases"]
    q20, q30 = one["q20_bases"] + two["q20_bases"], one["q30_bases"] + two["q30_bases"]
    return bases, {"total_reads": one["total_reads"] + two["total_reads"], "total_bases": bases, "q20_bases": q20, "q30_bases": q30, "q20_rate": _ratio(q20, bases),
                   "q30_rate": _ratio(q30, bases), "read1_mean_length": one["total_bases"] // one["total_reads"] if one["total_reads"] else 0,
                   "read2_mean_length": two["total_bases"] // two["total_reads"] if two["total_reads"] else 0}


def full_report(text1: bytes, text2: bytes, p, version: str, command: str):
    """the JSON of `-j` with `--full-report` as a dict (version: the library's palace_version(); command: the argument list, blanks between)"""
    res = rc.readqc(text1, text2, p)
    recs = (rc.records_of(text1), rc.records_of(text2))
    longest = [max([len(r[1]) for r in rs], default=0) for rs in recs]
    lens = (res["len1"], res["len2"])
    kept = int(np.sum(res["len1"] >= 0))
    blocks = {}
    for w in (0, 1):
        before, after = section(recs[w], None, longest[w]), section(recs[w], lens[w], longest[w])
        blocks[f"read{w + 1}_before_filtering"] = (_read_block(before, len(recs[w])), before)
        blocks[f"read{w + 1}_after_filtering"] = (_read_block(after, kept), after)
    summary = {"readqc_version": version,
               "sequencing": "paired end (%d cycles + %d cycles)" % (blocks["read1_before_filtering"][0]["total_cycles"], blocks["read2_before_filtering"][0]["total_cycles"])}
    for when in ("before_filtering", "after_filtering"):
        (one, s1), (two, s2) = blocks["read1_" + when], blocks["read2_" + when]
        bases, block = _summary_block(one, two)
        gc = sum(int(s["cnt"][:, k].sum()) for s in (s1, s2) for k in (1, 2))
        block["gc_content"] = _ratio(gc, bases)
        summary[when] = block
    hist = insert_histogram(text1, text2, p)
    small = rc.report(res)
    out = {"summary": summary, "filtering_result": dict(small["filtering_result"], too_long_reads=0), "adapter_cutting": small["adapter_cutting"],
           "insert_size": {"peak": int(np.argmax(hist[:ISIZE_MAX])), "unknown": int(hist[ISIZE_MAX]), "histogram": [int(x) for x in hist[:ISIZE_MAX]]}}
    out.update({k: blocks[k][0] for k in ("read1_before_filtering", "read2_before_filtering", "read1_after_filtering", "read2_after_filtering")})
    out["command"] = command
    return out


# ---- the hand-typed insert sizes -------------------------------------------------------------------------------------------------------
def insert_catalogue():
    """name -> (seq1, seq2, flags, candidate, slot), the last two typed by hand from the rules: F = max(0, L1 - 30) forward candidates
    (o, 0, min(L1 - o, L2)), then the reverse ones (0, k, min(L1, L2 - k))"""
    rng = np.random.default_rng(20261021)
    cat = {}
    frag = rc.random_seq(rng, 150)
    cat["forward_at_0"] = (frag, rc.revcomp(frag), "-", 0, 150)                                  # o = 0: the overlap is the fragment
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 151)
    cat["forward_at_1"] = (s1, s2, "-", 1, 151)                                                  # o = 1, n = 149: 150 + 150 - 149
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 200)
    cat["forward_at_50"] = (s1, s2, "-", 50, 200)
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 100)
    cat["reverse_k50"] = (s1, s2, "-", 120 + 50, 100)                                            # k = 50, n = 100: the fragment read through
    cat["reverse_k50_no_trim"] = (s1, s2, "A", -1, 512)
    s1 = rc.random_seq(rng, 30)
    cat["reverse_k0"] = (s1, rc.revcomp(s1 + rc.random_seq(rng, 120)), "-", 0, 30)               # no forward candidate: index 0 is k = 0
    cat["none"] = (b"AC" * 75, b"AC" * 75, "-", -1, 512)                                         # A: ACAC.., B: GTGT..: every position differs
    cat["too_short_to_search"] = (frag[:30], rc.revcomp(frag[:30]), "-", -1, 512)
    cat["empty_reads"] = (b"", b"", "-", -1, 512)
    for size in (511, 512, 513):                                                                 # reads of 300: o = size - 300, n = 600 - size
        s1, s2 = rc.pair_with_insert(rng, 300, 300, size)
        cat[f"clamp_{size}"] = (s1, s2, "-", size - 300, min(size, 512))
    return cat


# ---- the selftest's case lines ---------------------------------------------------------------------------------------------------------
def selftest_expected(kind: str, *fields) -> bytes:
    """I <flags> <seq1> <seq2> -> I <candidate> <slot>;  Q <hex of QUAL> <bases> -> Q <slot:value:q20:q30 per byte>"""
    if kind == "I":
        flags, s1, s2 = fields
        return b"I %d %d\n" % insert_size(s1.encode(), s2.encode(), rc.params(no_trim="A" in flags))
    assert kind == "Q"
    quals, bases = bytes.fromhex(fields[0]), fields[1].encode()
    return b"Q" + b"".join(b" %d:%d:%d:%d" % ((SLOTS.index(bytes([b])),) + qual_facts(q)) for q, b in zip(quals, bases)) + b"\n"
