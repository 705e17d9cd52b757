"""palace_fastq_records, palace_readqc_plan and palace_readqc_write (csrc/readqc.hip) through the C ABI against the Python restatement
of tests/readqc_cases.py -- never against the device's own output.  One text pair carries every hand-built case of the overlap search
and the filter; what a case is built to meet is asserted on the restatement first, so that the comparison cannot pass on cases that
miss their point."""
import numpy as np
import pytest

from palace_amd import capi, synth
from tests import readqc_cases as rc

pytestmark = pytest.mark.gpu

T = capi.SAM_TILE
GOOD = 33 + 40


def q(n, low=0, rng=None):
    return rc.qual_with_low(rng or synth.rng_for(n * 131 + low), n, low)


def build_cases():
    """name -> (seq1, qual1, seq2, qual2), and name -> what the restatement must say of it: (candidate index or None for "whatever",
    kept 1, kept 2, reason)"""
    rng = synth.rng_for(20261019)
    cases, want = {}, {}

    def add(name, s1, s2, expect, q1=None, q2=None):
        cases[name] = (s1, q1 if q1 is not None else bytes([GOOD]) * len(s1), s2, q2 if q2 is not None else bytes([GOOD]) * len(s2))
        want[name] = expect

    def rev_hit(l1, l2, insert):                                            # the reverse candidate k = l2 - insert in search order
        return max(0, l1 - 30) + l2 - insert

    # read lengths around every border of the rules and of a wavefront, alone and against a long mate
    for ln in (0, 1, 14, 15, 16, 29, 30, 31, 32, 49, 50, 51, 52, 63, 64, 65, 127, 128, 129, 150, 4096):
        s1, s2 = rc.pair_with_insert(rng, ln, ln, ln)
        add(f"len{ln}_full", s1, s2, (0 if ln > 30 else None, ln, ln, rc.PASS if ln >= 15 else rc.TOO_SHORT))
        s1, s2 = rc.pair_with_insert(rng, ln, 150, 60)
        add(f"len{ln}_vs150", s1, s2, None)
        s1, s2 = rc.pair_with_insert(rng, 150, ln, 60)
        add(f"150_vs_len{ln}", s1, s2, None)
    # inserts from 31 up to the read length: the reverse hit k = L - insert trims to the insert; insert = L is the forward hit o = 0
    for ins in range(31, 65):
        s1, s2 = rc.pair_with_insert(rng, 64, 64, ins)
        add(f"insert{ins}_of64", s1, s2, (rev_hit(64, 64, ins), ins, ins, rc.PASS) if ins < 64 else (0, 64, 64, rc.PASS))
    for ins in (31, 32, 49, 50, 51, 100, 149):
        s1, s2 = rc.pair_with_insert(rng, 150, 150, ins)
        add(f"insert{ins}_of150", s1, s2, (rev_hit(150, 150, ins), ins, ins, rc.PASS))
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 30)                          # k = 120 is not searched: k < L2 - 30
    add("insert30_of150", s1, s2, (-1, 150, 150, rc.PASS))
    # the limit, and where the count stops
    for name, mis, hit in (("limit", (3, 10, 20, 30, 40), True), ("limit_plus_1", (3, 10, 20, 30, 40, 45), False), ("sixth_at_49", (1, 2, 3, 4, 5, 49), False),
                           ("sixth_at_50", (1, 2, 3, 4, 5, 50), True), ("twenty_from_50", tuple(range(50, 70)), True),
                           ("five_and_twenty_from_50", (0, 12, 24, 36, 48) + tuple(range(50, 70)), True)):
        s1, s2 = rc.pair_with_insert(rng, 150, 150, 100, mismatches_at=mis)
        add(name, s1, s2, (rev_hit(150, 150, 100), 100, 100, rc.PASS) if hit else (-1, 150, 150, rc.PASS))
    # n = 24, 25, 26: the limit is 4, 5, 5 (n = L1 where read 1 is the shorter side)
    for n, limit in ((24, 4), (25, 5), (26, 5)):
        for extra in (0, 1):
            s1, s2 = rc.pair_with_insert(rng, n, 150, 60, mismatches_at=tuple(range(2, 2 + 3 * (limit + extra), 3)))
            add(f"n{n}_mis{limit + extra}", s1, s2, (90, n, n, rc.PASS) if not extra else (-1, n, 150, rc.PASS))
    # the accepted candidate at index 63, 64, 65 of the search order: forward, reverse, and where the two sides meet in one round of 64
    for o in (63, 64, 65):
        s1, s2 = rc.pair_with_insert(rng, 150, 150, 150 + o)
        add(f"forward_at_{o}", s1, s2, (o, 150, 150, rc.PASS))
        s1, s2 = rc.pair_with_insert(rng, 150, 150, 150 - o)
        add(f"reverse_k{o}", s1, s2, (120 + o, 150 - o, 150 - o, rc.PASS))
        s1, s2 = rc.pair_with_insert(rng, 50, 150, 150 - (o - 20))           # 20 forward candidates, then k = o - 20
        add(f"reverse_at_{o}", s1, s2, (o, 50, 50, rc.PASS))
    for o in (127, 128, 129):
        s1, s2 = rc.pair_with_insert(rng, 150, 150, 150 - (o - 120))
        add(f"reverse_at_{o}", s1, s2, (o, 270 - o, 270 - o, rc.PASS))
    # two acceptable candidates: the earlier wins although the later has fewer mismatches (a read of period 10)
    unit = b"ACGGTCATTG"
    noise = bytes(rc.other_base(c) for c in unit)
    marred = bytearray(unit)
    for at in (1, 4, 6, 9):
        marred[at] = rc.other_base(marred[at])
    a, b = unit * 15, noise + bytes(marred) + unit * 13                       # k = 10: 4 mismatches, n = 140; k = 20: none, n = 130
    add("earlier_wins", a, rc.revcomp(b), (120 + 10, 140, 140, rc.PASS))
    # a forward hit that blocks a reverse one that would trim
    add("forward_blocks_reverse", unit * 15, rc.revcomp(unit * 15), (0, 150, 150, rc.PASS))
    # k = 0 in reverse (read 1 of 30 bases has no forward candidate): accepted, never trims
    s1 = rc.random_seq(rng, 30)
    add("reverse_k0", s1, rc.revcomp(s1 + rc.random_seq(rng, 120)), (0, 30, 150, rc.PASS))
    # N against N is no mismatch: four N and two real mismatches in the window
    frag = bytearray(rc.random_seq(rng, 100))
    for at in (5, 15, 25, 35):
        frag[at] = ord("N")
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 100, mismatches_at=(8, 18), frag=bytes(frag))
    add("n_equals_n", s1, s2, (170, 100, 100, rc.PASS))
    # the filter's borders, counted over the kept prefix only (the tails behind it are as bad as can be)
    for name, low, nn, which, reason in (("low_at_border", 40, 0, 0, rc.PASS), ("low_over_border", 41, 0, 0, rc.LOW_QUALITY), ("low_at_border_r2", 40, 0, 1, rc.PASS),
                                         ("low_over_border_r2", 41, 0, 1, rc.LOW_QUALITY), ("five_n", 0, 5, 0, rc.PASS), ("six_n", 0, 6, 0, rc.TOO_MANY_N),
                                         ("five_n_r2", 0, 5, 1, rc.PASS), ("six_n_r2", 0, 6, 1, rc.TOO_MANY_N), ("low_before_n", 41, 6, 0, rc.LOW_QUALITY)):
        s1, s2 = rc.pair_with_insert(rng, 150, 150, 100)
        seqs, quals = [bytearray(s1), bytearray(s2)], [bytearray(bytes([GOOD]) * 150), bytearray(bytes([GOOD]) * 150)]
        quals[which][:100] = rc.qual_with_low(rng, 100, low)
        first = 60 if which == 0 else 10                                    # (behind the compared window: read 2's base q is the fragment's 99 - q)
        for at in range(first, first + nn):
            seqs[which][at] = ord("N")
        seqs[which][100:] = b"N" * 50                                        # (one read only: N tails on both would be an overlap of their own)
        for w in (0, 1):
            quals[w][100:] = bytes([33]) * 50
        add(name, bytes(seqs[0]), bytes(seqs[1]), (170, 100, 100, reason), bytes(quals[0]), bytes(quals[1]))
    # 14 and 15 bases after trimming
    for n in (14, 15):
        s1, s2 = rc.pair_with_insert(rng, n, 150, 60)
        add(f"trimmed_to_{n}", s1, s2, (90, n, n, rc.TOO_SHORT if n < 15 else rc.PASS))
    # read 2 fails where read 1 passes, and the other way round
    add("r1_short_r2_n", b"ACGT", b"N" * 40, (None, 4, 40, rc.TOO_SHORT))
    add("r1_ok_r2_n", rc.random_seq(rng, 40), b"N" * 40, (None, 40, 40, rc.TOO_MANY_N))
    return cases, want


CASES, WANT = build_cases()
NAMES = sorted(CASES)
SWITCHES = {"default": {}, "A": {"no_trim": 1}, "Q": {"no_quality_filter": 1}, "L": {"no_length_filter": 1}, "AQL": {"no_trim": 1, "no_quality_filter": 1, "no_length_filter": 1},
            "q20_u30_n3_l31": {"qualified_quality": 20, "unqualified_percent": 30, "n_limit": 3, "min_length": 31}}


def test_cases_meet_their_point():
    for name in NAMES:
        s1, q1, s2, q2 = CASES[name]
        if WANT[name] is None:
            continue
        c, _ = rc.overlap(s1, s2)
        got = (c,) + rc.run_pair((b"@", s1, b"+", q1), (b"@", s2, b"+", q2))
        assert got[1:] == WANT[name][1:] and WANT[name][0] in (None, got[0]), (name, got, WANT[name])
    s1, _, s2, _ = CASES["earlier_wins"]
    a, b = s1, rc.revcomp(s2)
    assert rc.accepted(a, b, (0, 20, 130), rc.DEFAULTS) and sum(x != y for x, y in zip(a[:50], b[20:70])) == 0
    s1, _, s2, _ = CASES["forward_blocks_reverse"]
    assert rc.accepted(s1, rc.revcomp(s2), (0, 10, 140), rc.DEFAULTS)


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


@pytest.fixture(scope="module")
def case_texts():
    return rc.texts_of([CASES[n] for n in NAMES], plus=b"+again")


@pytest.fixture(scope="module")
def case_run(ctx, case_texts):
    """the case texts on the device, planned with the defaults, and the restatement's result"""
    qc = capi.Readqc(ctx, *case_texts)
    want = rc.readqc(*case_texts)
    got = qc.plan()
    yield qc, got, want
    qc.close()


def same_plan(got, want, names=None):
    for k in ("len1", "len2"):
        bad = np.nonzero(got[k] != want[k])[0]
        assert len(bad) == 0, (k, [(names[i] if names else i, int(got[k][i]), int(want[k][i])) for i in bad[:8]])
    for k in ("off1", "off2"):
        assert np.array_equal(got[k], want[k]), k
    for k in rc.COUNTS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["bytes_1"] == len(want["out1"]) and got["bytes_2"] == len(want["out2"])


def test_records_of_the_case_texts(case_run, case_texts):
    qc, _, _ = case_run
    for (records, line, code, seq_len), text in zip(qc.records(), case_texts):
        assert (records, line, code) == rc.verdict(text) == (len(NAMES), 0, 0)
        assert np.array_equal(seq_len, [len(r[1]) for r in rc.records_of(text)])


def test_plan_of_the_case_texts(case_run):
    qc, got, want = case_run
    same_plan(got, want, NAMES)
    assert want["trimmed_reads"] > 100 and all(want[k] > 0 for k in rc.COUNTS)


@pytest.mark.parametrize("switch", [k for k in SWITCHES if k != "default"])
def test_switches_through_the_params(ctx, case_texts, switch):
    want = rc.readqc(*case_texts, rc.params(**SWITCHES[switch]))
    qc = capi.Readqc(ctx, *case_texts)
    try:
        got = qc.plan(capi.ReadqcParams.default(**SWITCHES[switch]))
        same_plan(got, want, NAMES)
        for w, key in enumerate(("out1", "out2")):
            assert qc.write(w, 0, len(want[key]))[32:-32] == want[key]
    finally:
        qc.close()
    base = rc.readqc(*case_texts)
    if "A" in switch:
        assert want["trimmed_reads"] == 0 < base["trimmed_reads"]
    if "Q" in switch:
        assert want["low_quality"] == want["too_many_n"] == 0 < base["low_quality"]
    if "L" in switch:
        assert want["too_short"] == 0 < base["too_short"]


def test_write_whole_range(case_run):
    qc, _, want = case_run
    for w, key in enumerate(("out1", "out2")):
        image = qc.write(w, 0, len(want[key]))
        assert image[32:-32] == want[key]
        assert image[:32] == image[-32:] == b"\xaa" * 32


def test_write_windows(case_run):
    """single bytes, windows cut at 15, 16 and 17 bytes and at record borders: the window's bytes and nothing else"""
    qc, _, want = case_run
    text, off = want["out1"], want["off1"]
    kept = [int(x) for x in np.unique(off)]
    windows = [(at, at + 1) for at in list(range(0, 40)) + kept[1:6] + [k - 1 for k in kept[1:6]] + [len(text) - 1]]
    for step in (15, 16, 17):
        windows += [(at, min(at + step, len(text))) for at in range(0, 40 * step, step)]
        windows += [(kept[3] - step, kept[3]), (kept[3], kept[3] + step), (kept[3] - 1, kept[3] + step), (len(text) - step, len(text))]
    windows += [(a, b) for a, b in zip(kept[:12], kept[1:13])] + [(kept[2], kept[9]), (kept[2] + 1, kept[9] - 1), (0, 0), (len(text), len(text)), (7, 7),
                                                                 (T - 1, 2 * T + 1), (1, T), (T, 2 * T), (5, 3 * T + 5)]
    for lo, hi in windows:
        image = qc.write(0, lo, hi)
        assert image[32:len(image) - 32] == text[lo:hi], (lo, hi)
        assert image[:32] == image[len(image) - 32:] == b"\xaa" * 32, (lo, hi)


def pad_to(records, at):
    """a name for the next record that puts the byte behind its name line at offset `at` of the text"""
    used = len(rc.fastq(records))
    return b"n" * (at - used - 2)


@pytest.mark.parametrize("delta", (-1, 0, 1))
def test_lines_and_records_around_tile_borders(ctx, delta):
    """every line of a record begins at T - 1, T or T + 1 in turn; a record of 4096 bases lies across tiles whatever is done"""
    rng = synth.rng_for(40 + delta)
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 100)
    for shift in (0, 151, 151 + 7, 151 + 7 + 151):                          # the name's end, SEQ's, the '+' line's, QUAL's at the border
        texts = []
        for seq in (s1, s2):
            head = [(b"first", rc.random_seq(rng, 40), bytes([GOOD]) * 40)]
            name = pad_to(head, T + delta - shift)
            texts.append(rc.fastq(head + [(name, seq, q(150, 10, rng), b"+again")] + [(b"last", rc.random_seq(rng, 33), bytes([GOOD]) * 33)]))
        want = rc.readqc(*texts)
        qc = capi.Readqc(ctx, *texts)
        try:
            assert [r[:3] for r in qc.records()] == [rc.verdict(t) for t in texts] == [(3, 0, 0)] * 2
            same_plan(qc.plan(), want)
            assert want["len1"][1] == 100
            for w, key in enumerate(("out1", "out2")):
                assert qc.write(w, 0, len(want[key]))[32:-32] == want[key]
        finally:
            qc.close()


def test_last_line_without_lf_and_empty_texts(ctx):
    rng = synth.rng_for(9)
    pairs = [rc.pair_with_insert(rng, 150, 150, 90) for _ in range(5)]
    t1, t2 = rc.texts_of([(a, bytes([GOOD]) * 150, b, bytes([GOOD]) * 150) for a, b in pairs])
    for texts in ((t1[:-1], t2), (t1, t2[:-1]), (t1[:-1], t2[:-1]), (b"", b"")):
        want = rc.readqc(*texts)
        qc = capi.Readqc(ctx, *texts)
        try:
            assert [r[:3] for r in qc.records()] == [rc.verdict(t) for t in texts] == [(len(want["len1"]), 0, 0)] * 2
            same_plan(qc.plan(), want)
            for w, key in enumerate(("out1", "out2")):
                assert qc.write(w, 0, len(want[key]))[32:-32] == want[key] and (not texts[0] or want[key].endswith(b"\n"))
        finally:
            qc.close()


def grammar_texts():
    good = [(b"g%d" % k, b"ACGTN" * 6, b"I" * 30) for k in range(3)]
    behind = rc.fastq([(b"behind", b"ACXT", b"I")])                          # a second fault behind the first: EBASE, and EQLEN behind that
    g = rc.fastq(good)

    def faulty(record_text):
        return g + record_text + behind

    long_ok, long_bad = b"A" * 4096, b"A" * 4097
    return {
        "eat": (faulty(b"x\nAC\n+\nII\n"), 13, rc.EAT), "eat_empty_name_line": (faulty(b"\nAC\n+\nII\n"), 13, rc.EAT),
        "eplus": (faulty(b"@x\nAC\n-\nII\n"), 15, rc.EPLUS), "eplus_empty": (faulty(b"@x\nAC\n\nII\n"), 15, rc.EPLUS),
        "elong": (faulty(b"@x\n" + long_bad + b"\n+\n" + b"I" * 4097 + b"\n"), 14, rc.ELONG), "long_ok": (g + rc.fastq([(b"x", long_ok, b"I" * 4096)]), 0, 0),
        "elong_before_ebase": (faulty(b"@x\n" + b"X" * 5000 + b"\n+\nI\n"), 14, rc.ELONG),
        "ebase_lower": (faulty(b"@x\nACgT\n+\nIIII\n"), 14, rc.EBASE), "ebase_cr": (faulty(b"@x\nACGT\r\n+\nIIIII\n"), 14, rc.EBASE),
        "ebase_far": (faulty(b"@x\n" + b"A" * 4000 + b"." + b"A" * 95 + b"\n+\n" + b"I" * 4096 + b"\n"), 14, rc.EBASE),
        "eqlen_short": (faulty(b"@x\nACGT\n+\nIII\n"), 16, rc.EQLEN), "eqlen_long": (faulty(b"@x\nACGT\n+\nIIIII\n"), 16, rc.EQLEN),
        "eqlen_before_equal": (faulty(b"@x\nACGT\n+\nII \n"), 16, rc.EQLEN),
        "equal_space": (faulty(b"@x\nACGT\n+\nII I\n"), 16, rc.EQUAL), "equal_del": (faulty(b"@x\nACGT\n+\nIII\x7f\n"), 16, rc.EQUAL),
        "equal_cr": (faulty(b"@x\nACGT\n+\nIII\r\n"), 16, rc.EQUAL), "equal_far": (faulty(b"@x\n" + long_ok + b"\n+\n" + b"I" * 4095 + b"\x80\n"), 16, rc.EQUAL),
        "qual_borders_ok": (g + rc.fastq([(b"x", b"AC", b"!~")]), 0, 0),
        "elines_1": (g + b"@x\n", 13, rc.ELINES), "elines_2": (g + b"@x\nAC\n", 13, rc.ELINES), "elines_3": (g + b"@x\nAC\n+\nII\n@y\nAC\n+", 17, rc.ELINES),
        "elines_blank_end": (g + b"\n", 13, rc.ELINES), "elines_only_lf": (b"\n", 1, rc.ELINES), "fault_before_elines": (faulty(b"") + b"@x\n", 14, rc.EBASE),
        "first_line": (b"x" + g, 1, rc.EAT), "empty": (b"", 0, 0), "valid": (g, 0, 0), "valid_no_lf": (g[:-1], 0, 0),
    }


def test_every_grammar_code_at_the_smallest_line(ctx):
    cases = grammar_texts()
    names = sorted(cases)
    assert {cases[n][2] for n in names} == set(range(8))
    for n in names:
        text, line, code = cases[n]
        assert rc.verdict(text)[1:] == (line, code), n
    if len(names) % 2:
        names.append(names[0])
    for a, b in zip(names[::2], names[1::2]):
        qc = capi.Readqc(ctx, cases[a][0], cases[b][0])
        try:
            got = qc.records()
            for n, r in zip((a, b), got):
                assert r[:3] == rc.verdict(cases[n][0]), n
        finally:
            qc.close()


def test_unequal_record_counts(ctx):
    t1, t2 = rc.fastq([(b"a", b"ACGT", b"IIII")] * 3), rc.fastq([(b"a", b"ACGT", b"IIII")] * 2)
    qc = capi.Readqc(ctx, t1, t2)
    try:
        assert [r[:3] for r in qc.records()] == [(3, 0, 0), (2, 0, 0)]
    finally:
        qc.close()


def test_seeded_random_text(ctx):
    rng = synth.rng_for(77)
    pairs = rc.random_pairs(rng, 2500)
    texts = rc.texts_of(pairs)
    want = rc.readqc(*texts)
    assert want["reads_after"] > 1000 and want["trimmed_reads"] > 200 and min(want["low_quality"], want["too_many_n"], want["too_short"]) > 50
    qc = capi.Readqc(ctx, *texts)
    try:
        assert [r[:3] for r in qc.records()] == [(2500, 0, 0)] * 2
        same_plan(qc.plan(), want)
        for w, key in enumerate(("out1", "out2")):
            assert qc.write(w, 0, len(want[key]))[32:-32] == want[key]
            cut = len(want[key]) // 3 + 5
            assert qc.write(w, cut, 2 * cut)[32:-32] == want[key][cut:2 * cut]
    finally:
        qc.close()
