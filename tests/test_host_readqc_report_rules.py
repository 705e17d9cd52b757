"""The rules of `readqc --full-report` (DESIGN.md 8 "Reports") on a CPU: a hand-typed catalogue pins the restatement of
tests/readqc_report_cases.py, and the `I` (insert size) and `Q` (QUAL byte, base slot) kinds of the stand-alone `fastq_rules_selftest` --
as built and under ASan + UBSan -- equal the restatement on the catalogue and on seeded pairs.  (The kernels:
tests/test_gpu_readqc_report_abi.py; the tool: tests/test_gpu_readqc_report_cli.py.)"""
import os
import subprocess

import numpy as np
import pytest

from palace_amd import synth
from tests import readqc_cases as rc
from tests import readqc_report_cases as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = ("fastq_rules_selftest", "fastq_rules_selftest_asan")

# QUAL byte -> (value, Q20, Q30), typed by hand
QUAL_BY_HAND = {33: (0, False, False), 52: (19, False, False), 53: (20, True, False), 62: (29, True, False), 63: (30, True, True), 126: (93, True, True)}

def test_qual_bytes_by_hand():
    for q, want in QUAL_BY_HAND.items():
        assert rr.qual_facts(q) == want, q
    sec = rr.section([(b"@", b"ACGTNA", b"+", bytes(sorted(QUAL_BY_HAND)))], None, 6)
    assert (sec["q20"], sec["q30"]) == (4, 2)
    assert sec["qsum"].sum(axis=1).tolist() == [0, 19, 20, 29, 30, 93]


def test_a_read_of_every_base_by_hand():
    sec = rr.section([(b"@", b"ACGTN", b"+", b"5?I!~")], None, 7)           # QUAL 20, 30, 40, 0, 93
    assert sec["cnt"].tolist() == [[1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [0, 0, 1, 0, 0], [0, 0, 0, 1, 0], [0, 0, 0, 0, 1], [0] * 5, [0] * 5]
    assert sec["qsum"].tolist() == [[20, 0, 0, 0, 0], [0, 30, 0, 0, 0], [0, 0, 40, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 93], [0] * 5, [0] * 5]
    assert (sec["q20"], sec["q30"]) == (4, 3)
    two = [(b"@", b"ACGTN", b"+", b"5?I!~"), (b"@", b"AAA", b"+", b"III")]
    cut = rr.section(two, [2, -1], 5)                                        # the first read's two first cycles, nothing of a dropped read
    assert cut["cnt"].sum() == 2 and cut["qsum"].sum() == 50 and (cut["q20"], cut["q30"]) == (2, 1)
    short = rr.section(two, None, 2)                                         # cycles >= max_cycles are not counted
    assert short["cnt"].tolist() == [[2, 0, 0, 0, 0], [1, 1, 0, 0, 0]] and short["qsum"].tolist() == [[60, 0, 0, 0, 0], [40, 30, 0, 0, 0]]


def test_insert_sizes_by_hand():
    for name, (s1, s2, flags, c, slot) in rr.insert_catalogue().items():
        assert rr.insert_size(s1, s2, rc.params(no_trim="A" in flags)) == (c, slot), name


def test_report_of_a_tiny_text_by_hand():
    t1 = rc.fastq([(b"a", b"ACGT" * 5, b"I" * 20), (b"b", b"GG", b"5!")])
    t2 = rc.fastq([(b"a", b"TTTTT" * 4 + b"N", b"?" * 21), (b"b", b"C", b"!")])
    rep = rr.full_report(t1, t2, rc.DEFAULTS, "v", "cmd")
    before, after = rep["summary"]["before_filtering"], rep["summary"]["after_filtering"]
    assert before == {"total_reads": 4, "total_bases": 44, "q20_bases": 42, "q30_bases": 41, "q20_rate": 42 / 44, "q30_rate": 41 / 44, "read1_mean_length": 11,
                      "read2_mean_length": 11, "gc_content": 13 / 44}
    assert after["total_reads"] == 2 and after["total_bases"] == 41 and after["read1_mean_length"] == 20 and after["read2_mean_length"] == 21       # pair b: one low byte of two
    assert rep["summary"]["sequencing"] == "paired end (20 cycles + 21 cycles)" and rep["command"] == "cmd" and rep["summary"]["readqc_version"] == "v"
    assert rep["filtering_result"] == {"passed_filter_reads": 2, "low_quality_reads": 2, "too_many_N_reads": 0, "too_short_reads": 0, "too_long_reads": 0}
    assert rep["insert_size"]["unknown"] == 2 and rep["insert_size"]["peak"] == 0 and rep["insert_size"]["histogram"] == [0] * 512
    r1 = rep["read1_before_filtering"]
    assert r1["total_cycles"] == 20 and r1["total_reads"] == 2 and r1["total_bases"] == 22
    assert r1["content_curves"]["A"][:2] == [0.5, 0.0] and r1["content_curves"]["G"][:2] == [0.5, 0.5] and r1["content_curves"]["GC"][:3] == [0.5, 1.0, 1.0]
    assert r1["quality_curves"]["G"][:3] == [20.0, 0.0, 40.0] and r1["quality_curves"]["mean"][:3] == [30.0, 20.0, 40.0] and r1["quality_curves"]["T"][:3] == [0.0, 0.0, 0.0]
    assert len(r1["quality_curves"]["mean"]) == len(r1["content_curves"]["N"]) == 20
    r2 = rep["read2_after_filtering"]
    assert r2["total_cycles"] == 21 and r2["total_reads"] == 1 and r2["content_curves"]["N"][20] == 1.0 and r2["quality_curves"]["mean"] == [30.0] * 21
    empty = rr.full_report(b"", b"", rc.DEFAULTS, "v", "cmd")
    assert empty["summary"]["before_filtering"]["gc_content"] == 0.0 and empty["read1_after_filtering"]["quality_curves"]["mean"] == []


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in TOOLS], check=True, stdout=subprocess.DEVNULL)


def case_file():
    cases = [("I", flags, s1.decode(), s2.decode()) for s1, s2, flags, _, _ in rr.insert_catalogue().values()]
    rng = synth.rng_for(4242)
    for k, p in enumerate(rc.random_pairs(rng, 5000)):
        cases.append(("I", "A" if k % 97 == 0 else "-", p[0].decode(), p[2].decode()))
    cases.append(("Q", bytes(sorted(QUAL_BY_HAND)).hex(), "ACGTNA"))
    cases.append(("Q", bytes(range(33, 127)).hex(), ("ACGTN" * 19)[:94]))
    cases.append(("Q", "", ""))
    return cases


@pytest.mark.parametrize("tool", TOOLS)
def test_rules_header_against_the_restatement(built, tmp_path, tool):
    cases = case_file()
    (tmp_path / "cases.txt").write_bytes(b"".join(rc.selftest_line(*c) for c in cases))
    p = subprocess.run([os.path.join(BIN, tool), str(tmp_path / "cases.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr
    got, want = p.stdout.splitlines(keepends=True), [rr.selftest_expected(*c[:1], *c[1:]) for c in cases]
    assert len(got) == len(want)
    for c, g, w in zip(cases, got, want):
        assert g == w, (c, g, w)
    slots = np.array([int(w.split()[2]) for w in want if w.startswith(b"I")])
    forward = sum(1 for c, w in zip(cases, want) if w.startswith(b"I") and 1 <= int(w.split()[1]) < max(0, len(c[2]) - 30))
    assert np.sum(slots == 512) > 500 and np.sum(slots < 150) > 500 and forward > 300     # unknown, read-through and longer fragments are all met
