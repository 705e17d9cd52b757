"""The rules of filter_result on the host: the Python restatement of tests/filter_result_cases.py against what the reference's script
itself wrote (tests/golden/filter_result_cases.npz; PINNED: the BLAST groups, the score and hit rules, which paths are written, the
first-occurrence rule, the tagged stdout lines, the cycle file's lines; UNPINNED: the FASTA reader and the complement table, which are
a stand-in's where the golden file is made; DECLARED: the cycle file is compared as a sorted list of lines, the two prints of Python
objects are dropped from stdout), what the catalogue reaches, the integer forms the device decides against the literal form, and the
search of the identity cuts -- the executable's own function, reached through `blast_line_selftest cuts` -- against float()."""
import collections
import os
import subprocess

import numpy as np
import pytest

from tests import filter_result_cases as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
TOOL = os.path.join(ROOT, "palace_amd", "bin", "blast_line_selftest")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "blast_line_selftest")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "filter_result_cases.npz"))


@pytest.fixture(scope="module")
def results():
    return {name: fr.filter_result(*case) for name, case in fr.golden_inputs().items()}


def tagged(stdout: bytes):
    """stdout without the two prints of Python objects: the lines that begin with one of the four words"""
    return [line for line in stdout.split(b"\n") if line.startswith(fr.TAGGED)]


def test_restatement_against_hand_worked_cases():
    fr.hand_checks()


def test_restatement_equals_the_reference_on_every_golden_case(golden, results):
    cases = fr.golden_inputs()
    assert len(cases) >= 20 and {k.split("__")[0] for k in golden.files} == set(cases)
    for name, (fasta, paths, blast, ratio, hits, scores) in cases.items():
        for key, val in (("fasta", fasta), ("paths", paths), ("blast", blast), ("hits", hits), ("scores", scores)):
            assert golden[f"{name}__{key}"].tobytes() == val, (name, key)          # the inputs the reference saw are the catalogue's
        assert golden[name + "__args"].tobytes().split(b"\0")[4] == ratio, name
        res = results[name]
        assert res.fasta == golden[name + "__out"].tobytes(), name
        assert res.said == tagged(golden[name + "__stdout"].tobytes()), name
        assert sorted(res.cycle) == sorted(golden[name + "__cycle"].tobytes().split(b"\n")[:-1]), name


def test_what_the_catalogue_reaches(results):
    cases = fr.golden_inputs()
    total = collections.Counter()
    for res in results.values():
        total += res.cover
    for key in ("first_line_fails", "first_line_passes", "group_start_fails", "group_start_passes", "inside_fails", "inside_passes", "group_flagged",
                "group_not_flagged", "group_at_ratio", "query_with_two_subjects", "empty_table",                                  # the BLAST groups, both sides
                "score_0.7", "score_0.70000001", "score_0.9", "score_0.8999", "score_below", "score_lower_second_ignored", "score_replaced_lower",
                "header_before_paths", "header_after_paths", "blank_line", "path_tags_00", "path_tags_10", "path_tags_01", "path_tags_11",
                "multi_token_under_self", "single_self", "single_self_under_cycle", "single_token_not_self", "selfgene_by_gene", "selfgene_by_score",
                "self_plain", "cycle_gene", "cycle_no_gene", "cycle_score", "cycle_no_score", "flags_by_blast", "blast_share_at_0.2", "dropped_no_score",
                "dropped_short", "kept_by_flags", "kept_by_score_and_length", "write_first", "write_again", "cycle_line", "cycle_short", "all_len_999",
                "all_len_1000", "all_len_9999", "all_len_10000"):
        assert total[key] > 0, key
    assert {case[3] for case in cases.values()} >= {b"0.75", b"0.7"}
    # the edges case by itself: 75 / 100 at 0.75 and 7 / 10 at 0.7 are not above the ratio, one step more is
    lengths = {k: len(v) for k, v in fr.parse_fasta(cases["edges_075"][0]).items()}
    seg75 = fr.blast_groups(cases["edges_075"][2], lengths, 0.75)[2]
    seg70 = fr.blast_groups(cases["edges_07"][2], lengths, 0.7)[2]
    assert seg75 == {b"c100", b"e1", b"v10"} and seg70 == seg75 | {b"u10", b"NODE_7_length_12_cov_1.5"} and b"t10" not in seg70       # (9 / 12 is 0.75)
    # equal lines that differ only in class: the first WRITER is written, not the first occurrence
    res = results["edges_075"]
    x = [k for k, j in enumerate(res.joined) if j == b"x20+"]
    assert [res.classes[k] for k in x[:2]] == [0, fr.WRITE | fr.PLAIN] and res.fasta.count(b">x20+\n") == 1
    c = [k for k, j in enumerate(res.joined) if j == b"c100+"]
    assert [res.classes[k] for k in c] == [fr.WRITE, fr.WRITE | fr.PLAIN] and res.fasta.count(b">c100+\n") == 1
    # 0.95 then 0.5 keeps 0.95; 0.95 then 0.8 -- at least 0.7, so the script stores it -- loses the 0.9 (the reference decides: see the golden)
    assert b"cyclescoredd+d950+" in res.said and b"cyclescorede+d950+" not in res.said


def test_integer_forms_equal_the_literal_form(results):
    """path_class from a path's facts and outputs_from_classes from classes + first_of_equal: what the device and the executable compute"""
    n = 0
    for name, (fasta, paths, blast, ratio, hits, scores) in fr.golden_inputs().items():
        res = results[name]
        lengths = {k: len(v) for k, v in fr.parse_fasta(fasta).items()}
        segs = fr.blast_groups(blast, lengths, float(ratio))[2]
        score, gene = fr.read_scores(scores), set(fr.read_hits(hits))
        for joined, tag, cls, all_len in zip(res.joined, res.tags, res.classes, res.all_len):
            names = [t for t in fr.re.split(rb"[+-]", joined) if t]
            facts = (len(names), tag, any(t in gene for t in names), any(score.get(t, 0) > 0.7 for t in names), any(score.get(t, 0) >= 0.9 for t in names),
                     sum(lengths[t] for t in names), sum(lengths[t] for t in names if t in segs))
            assert facts[5] == all_len and fr.path_class(*facts) == cls, (name, joined)
            n += 1
        written, said, cycle = fr.outputs_from_classes(res)
        assert (said, cycle) == (res.said, res.cycle) and written == [rec.split(b"\n")[0] for rec in res.fasta.split(b">")[1:]], name
    assert n > 400


@pytest.mark.parametrize("ratio", ["0.75", "0.7", "0.29"])
def test_identity_cuts_against_float(ratio):
    p = subprocess.run([TOOL, "cuts", ratio], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and p.stderr == b""
    cuts = [int(v) for v in p.stdout.split()]
    threshold = float(ratio) * 100
    assert cuts == fr.identity_cuts(threshold) and len(cuts) == 7
    for k, cut in enumerate(cuts):
        for value in (cut - 1, cut, cut + 1):
            digits = "%0*d" % (k + 1, value)
            text = digits if k == 0 else digits[:-k] + "." + digits[-k:]
            assert fr.blast_line(b"q\ts\t" + text.encode() + b"\t1") == ("L", value, k, 1), text
            assert (float(text) > threshold) == (value >= cut), (ratio, text)
