"""palace_amd/scripts/phage_scoring.py as the driver starts it: the lines it writes, its score format, and its faults."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import contig_feature_cases as cc
from tests import scorer_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "phage_scoring.py")


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("phage_scoring")
    torch.save(sc.checkpoint(), str(d / "model.pt"))
    text, _ = cc.fasta([(name + b" length=%d" % len(seq), seq) for name, seq in sc.scorer_contigs()])
    (d / "contigs.fasta").write_bytes(text)
    return d


def run(work, fasta, out, model="model.pt", batch=None):
    args = [sys.executable, SCRIPT, str(work / fasta), str(work / out), "0", "8", str(work / model)] + ([str(batch)] if batch else [])
    return subprocess.run(args, capture_output=True, text=True, timeout=300)


def parsed(path):
    data = path.read_bytes()
    assert data and not data.endswith(b"\n")
    names, scores = [], []
    for line in data.decode().split("\n"):
        name, score = line.split("\t")
        assert re.fullmatch(r"[0-9.e+-]+|nan", score) and score == format(np.float32(score), ""), score
        names.append(name)
        scores.append(float(np.float32(score)))
    return names, np.array(scores)


@pytest.fixture(scope="module")
def scored(work):
    p = run(work, "contigs.fasta", "scores.out")
    assert p.returncode == 0, p.stderr
    assert not (work / "scores.out.tmp").exists()
    return parsed(work / "scores.out")


def test_names_and_scores(scored):
    names, scores = scored
    assert names == [n.decode() for n, _ in sc.scorer_contigs()]               # the name ends at the header's first blank
    want = sc.reference()[2]
    # the text holds the shortest digits that give the float32 back, so reading it adds nothing to the device's distance
    worst = np.abs(scores - want).max()
    print("script against literal float64: scores", worst, "allowed", sc.TOL_SCORES)
    assert worst <= sc.TOL_SCORES


def test_window_of_one_record(work, scored):
    p = run(work, "contigs.fasta", "scores_1.out", batch=1)
    assert p.returncode == 0, p.stderr
    names, scores = parsed(work / "scores_1.out")
    assert names == scored[0]
    worst = np.abs(scores - scored[1]).max()
    print("batch_size 1 against 1000: scores", worst)
    assert worst <= sc.TOL_SCORES


def test_empty_fasta(work):
    (work / "empty.fasta").write_bytes(b"")
    p = run(work, "empty.fasta", "empty.out")
    assert p.returncode == 0, p.stderr
    assert (work / "empty.out").read_bytes() == b"" and not (work / "empty.out.tmp").exists()


def refused(work, p, out, message):
    assert p.returncode == 1 and p.stdout == ""
    assert p.stderr.strip().splitlines()[-1] == message, p.stderr
    assert not (work / out).exists() and not (work / (out + ".tmp")).exists()


def test_digit_in_a_sequence(work):
    text, _ = cc.fasta([(b"c1_length_500", cc.dna(np.random.default_rng(5), 500)), (b"c2", b"ACGTACGTAC" * 7 + b"ACG7ACGT")])
    (work / "digit.fasta").write_bytes(text)
    assert text.split(b"\n")[12].startswith(b"ACGTACGTACACG7")          # line 13: the second line of c2's sequence
    refused(work, run(work, "digit.fasta", "digit.out"), "digit.out", f"phage_scoring: {work / 'digit.fasta'}: line 13: digit in sequence")


def test_missing_key(work):
    torch.save({}, str(work / "no_keys.pt"))         # the keys are asked for in the model's order: the first is named
    refused(work, run(work, "contigs.fasta", "nokey.out", model="no_keys.pt"), "nokey.out", "phage_scoring: model: key pnode_d.weight is missing")


def test_index_fault(work):
    (work / "ragged.fasta").write_bytes(b">a\nACGT\nACGTAC\nAC\n")
    refused(work, run(work, "ragged.fasta", "ragged.out"), "ragged.out",
            f"phage_scoring: {work / 'ragged.fasta'}: line 3: a sequence line behind a line of another length than the record's first "
            "(only a record's last line may be shorter)")
