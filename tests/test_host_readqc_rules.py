"""The rules of `readqc` on a CPU: the restatement's "first 50" overlap against the literal loop it was derived from;
csrc/fastq_rules.hpp -- driven by the stand-alone `fastq_rules_selftest`, as built and under ASan + UBSan -- against the restatement
of tests/readqc_cases.py; and the filter's borders.  (The kernels: tests/test_gpu_readqc.py; the tool: tests/test_gpu_readqc_cli.py.)"""
import os
import subprocess

import pytest

from palace_amd import synth
from tests import readqc_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = ("fastq_rules_selftest", "fastq_rules_selftest_asan")
LENGTHS = (0, 1, 29, 30, 31, 32, 49, 50, 51, 52, 64, 65, 100, 150)


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in TOOLS], check=True, stdout=subprocess.DEVNULL)


def seeded_pair(rng):
    """lengths from LENGTHS; half of the pairs come from one fragment, with mismatches spread over the whole overlap so that both sides
    of position 50 and both sides of the limit are met"""
    l1, l2 = (int(rng.choice(LENGTHS)) for _ in range(2))
    if rng.random() < 0.5 or min(l1, l2) == 0:
        return rc.random_seq(rng, l1), rc.random_seq(rng, l2)
    insert = int(rng.integers(1, l1 + l2 + 1))
    n_mis = int(rng.integers(0, 9)) if rng.random() < 0.7 else int(rng.integers(9, 40))
    return rc.pair_with_insert(rng, l1, l2, insert, mismatches_at=[int(x) for x in rng.integers(0, max(1, insert), size=n_mis)])


def test_first_50_form_equals_the_literal_loop():
    rng = synth.rng_for(20261019)
    n, hits = 20000, 0
    for _ in range(n):
        s1, s2 = seeded_pair(rng)
        c, cand = rc.overlap(s1, s2)
        lit = rc.literal_overlap(s1, s2)
        if cand is None:
            assert lit is None, (s1, s2)
            continue
        hits += 1
        a0, b0, m = cand
        assert lit == (a0 if b0 == 0 else -b0, m), (s1, s2, cand, lit)
    print(f"accepted overlaps: {hits} of {n}")
    assert hits * 5 >= n                                                    # the test cannot pass on misses alone


def test_pair_builder_gives_the_overlap_it_names():
    rng = synth.rng_for(5)
    for l1, l2, insert in ((150, 150, 100), (150, 150, 31), (100, 150, 60), (150, 100, 99), (64, 65, 40)):
        s1, s2 = rc.pair_with_insert(rng, l1, l2, insert)
        f = max(0, l1 - 30)
        assert rc.overlap(s1, s2) == (f + l2 - insert, (0, l2 - insert, insert)) and rc.trim_to(s1, s2) == insert
    s1, s2 = rc.pair_with_insert(rng, 150, 150, 200)                         # a fragment longer than a read: forward, nothing trimmed
    assert rc.overlap(s1, s2) == (50, (50, 0, 100)) and rc.trim_to(s1, s2) is None


def case_file(rng):
    hexq = lambda q: q.hex()
    cases = []
    good = rc.fastq([(b"a", b"ACGTN", b"IIIII"), (b"b c", b"", b"")])
    texts = [b"", b"\n", good, good[:-1], good + b"@x\nAC\n+\n", good.replace(b"@b", b"b"), good.replace(b"+\nIIIII", b"-\nIIIII"), good.replace(b"ACGTN", b"ACGTn"),
             good.replace(b"ACGTN", b"ACGT\r"), good.replace(b"IIIII", b"IIII"), good.replace(b"IIIII", b"III I"), good.replace(b"IIIII", b"III\x7f"),
             good.replace(b"IIIII", b"IIII\r"), good.replace(b"\n", b"\r\n"), good + b"\n", b"\n" + good, rc.fastq([(b"l", b"A" * 4096, b"I" * 4096)]),
             rc.fastq([(b"ok", b"A", b"I"), (b"l", b"A" * 4097, b"I" * 4097)]), rc.fastq([(b"two", b"ACXT", b"II")]), b"@only\nAC"]
    for t in texts:
        cases.append(("G", t.hex()))
    for _ in range(300):
        s1, s2 = seeded_pair(rng)
        q1, q2 = (rc.qual_with_low(rng, len(s), int(rng.integers(0, len(s) + 1)) if rng.random() < 0.4 else 0) for s in (s1, s2))
        flags = "".join(f for f in "AQL" if rng.random() < 0.15) or "-"
        cases.append(("P", flags, s1.decode(), hexq(q1), s2.decode(), hexq(q2)))
    for ln, low in ((100, 40), (100, 41), (15, 6), (15, 7), (14, 0), (15, 0), (0, 0)):
        cases.append(("P", "-", "A" * ln, hexq(rc.qual_with_low(rng, ln, low)), "C" * 40, hexq(b"I" * 40)))
    for nn in (5, 6):
        cases.append(("P", "-", "N" * nn + "A" * 30, hexq(b"I" * (30 + nn)), "C" * 40, hexq(b"I" * 40)))
    return cases


@pytest.mark.parametrize("tool", TOOLS)
def test_rules_header_against_the_restatement(built, tmp_path, tool):
    cases = case_file(synth.rng_for(77))
    (tmp_path / "cases.txt").write_bytes(b"".join(rc.selftest_line(*c) for c in cases))
    p = subprocess.run([os.path.join(BIN, tool), str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr
    got, want = p.stdout.splitlines(keepends=True), [rc.selftest_expected(*c) for c in cases]
    assert len(got) == len(want)
    for c, g, w in zip(cases, got, want):
        assert g == w, c
    kinds = {w.split()[-1] for w in want if w.startswith(b"P")}
    assert kinds == {b"0", b"1", b"2", b"3"}                                # every reason is met
    assert {int(w.split()[3]) for w in want if w.startswith(b"G")} == set(range(8))          # ... and every grammar code


def test_grammar_by_hand():
    good = rc.fastq([(b"a", b"ACGTN", b"IIIII"), (b"b", b"", b"")])
    one = rc.fastq([(b"a", b"ACGTN", b"IIIII")])
    assert rc.verdict(b"") == (0, 0, 0) and rc.verdict(good) == (2, 0, 0) and rc.verdict(one[:-1]) == (1, 0, 0)        # a last line without LF is a line
    assert rc.verdict(good[:-1]) == (1, 5, rc.ELINES)                        # ... but an empty one is not: the text ends behind the '+' line's LF
    assert rc.verdict(b"\n") == (0, 1, rc.ELINES) and rc.verdict(good + b"\n") == (2, 9, rc.ELINES)
    assert rc.verdict(b"\n" + good) == (2, 1, rc.EAT)
    assert rc.verdict(good.replace(b"\n", b"\r\n")) == (2, 2, rc.EBASE)                      # CR is a byte like any other
    assert rc.verdict(good.replace(b"IIIII", b"IIII\r")) == (2, 4, rc.EQUAL)
    two = rc.fastq([(b"a", b"ACXT", b"II"), (b"b", b"A", b"I", b"x")])                       # the smallest line wins, and a line's first code
    assert rc.verdict(two) == (2, 2, rc.EBASE)
    assert rc.verdict(rc.fastq([(b"l", b"X" * 4097, b"I")])) == (1, 2, rc.ELONG)


def test_filter_borders():
    rng = synth.rng_for(3)
    q = lambda ln, low: rc.qual_with_low(rng, ln, low)
    assert rc.read_filter(b"A" * 100, q(100, 40)) == rc.PASS and rc.read_filter(b"A" * 100, q(100, 41)) == rc.LOW_QUALITY       # low * 100 == 40 * L passes
    assert rc.read_filter(b"A" * 15, q(15, 6)) == rc.PASS and rc.read_filter(b"A" * 15, q(15, 7)) == rc.LOW_QUALITY
    assert rc.read_filter(b"N" * 5 + b"A" * 20, b"I" * 25) == rc.PASS and rc.read_filter(b"N" * 6 + b"A" * 20, b"I" * 25) == rc.TOO_MANY_N
    assert rc.read_filter(b"A" * 14, b"I" * 14) == rc.TOO_SHORT and rc.read_filter(b"A" * 15, b"I" * 15) == rc.PASS
    assert rc.read_filter(b"", b"") == rc.TOO_SHORT
    # the order: low quality before N before length
    assert rc.read_filter(b"N" * 10, q(10, 10)) == rc.LOW_QUALITY and rc.read_filter(b"N" * 10, b"I" * 10) == rc.TOO_MANY_N
    # the switches
    assert rc.read_filter(b"N" * 10, q(10, 10), rc.params(no_quality_filter=1)) == rc.TOO_SHORT
    assert rc.read_filter(b"A" * 3, b"I" * 3, rc.params(no_length_filter=1)) == rc.PASS
    # a byte at the threshold is not low: 33 + 15 counts as good
    assert rc.read_filter(b"A" * 20, bytes([33 + 15]) * 20) == rc.PASS and rc.read_filter(b"A" * 20, bytes([33 + 14]) * 20) == rc.LOW_QUALITY
    # a pair counts under read 1's reason, or read 2's when read 1 passes
    bad_n, short, ok = (b"@", b"N" * 20, b"+", b"I" * 20), (b"@", b"A" * 3, b"+", b"I" * 3), (b"@", b"A" * 20, b"+", b"I" * 20)
    assert rc.run_pair(bad_n, short)[2] == rc.TOO_MANY_N and rc.run_pair(short, bad_n)[2] == rc.TOO_SHORT and rc.run_pair(ok, bad_n)[2] == rc.TOO_MANY_N
