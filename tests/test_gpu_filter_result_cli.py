"""bin/filter_result and scripts/filter_result.py: every case of tests/golden/filter_result_cases.npz (what the reference's script
itself wrote; PINNED: the BLAST groups, the score and hit rules, which paths are written, the first-occurrence rule, the tagged stdout
lines, the cycle file's lines; UNPINNED: the FASTA reader and the complement table, a stand-in's where the golden file is made;
DECLARED: the cycle file is compared as a sorted list of lines, the two prints of Python objects are dropped from the reference's
stdout) through the executable and through the script, the output window, and the declared faults."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import filter_result_cases as fr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "palace_amd", "bin", "filter_result")
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "filter_result.py")
FILES = {"fasta": "asm.fasta", "paths": "all_result.txt", "blast": "hits.blast", "hits": "gene_hit.txt", "scores": "node_score.txt"}
OUTPUTS = ("filtered.fasta", "filtered_cycle.txt")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "filter_result_cases.npz"))


def write_inputs(d, case, missing=None):
    fasta, paths, blast, ratio, hits, scores = case
    for key, text in (("fasta", fasta), ("paths", paths), ("blast", blast), ("hits", hits), ("scores", scores)):
        if key != missing:
            (d / FILES[key]).write_bytes(text)
    return [FILES["fasta"], FILES["paths"], OUTPUTS[0], FILES["blast"], ratio.decode(), FILES["hits"], FILES["scores"], OUTPUTS[1]]


def run(cmd, d, words, env=None):
    p = subprocess.run(cmd + words, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr


def tagged(stdout: bytes):
    return [line for line in stdout.split(b"\n") if line.startswith(fr.TAGGED)]


def compare(d, name, golden, out):
    assert (d / OUTPUTS[0]).read_bytes() == golden[name + "__out"].tobytes(), name
    assert out.split(b"\n")[:-1] == tagged(golden[name + "__stdout"].tobytes()), name
    assert sorted((d / OUTPUTS[1]).read_bytes().split(b"\n")[:-1]) == sorted(golden[name + "__cycle"].tobytes().split(b"\n")[:-1]), name
    assert not any((d / (o + ".tmp")).exists() for o in OUTPUTS)


@pytest.mark.parametrize("how", ["binary", "script"])
def test_every_golden_case(how, golden, tmp_path):
    cmd = [BINARY] if how == "binary" else [sys.executable, SCRIPT]
    for name, case in fr.golden_inputs().items():
        d = tmp_path / name
        d.mkdir()
        rc, out, err = run(cmd, d, write_inputs(d, case))
        assert (rc, err) == (0, b""), (name, rc, err[-600:])
        compare(d, name, golden, out)
        assert (d / OUTPUTS[1]).read_bytes().split(b"\n")[:-1] == fr.filter_result(*case).cycle, name       # and in the declared order


@pytest.mark.parametrize("case", ["edges_075", "random_13"])
def test_the_output_window_does_not_show(case, golden, tmp_path):
    words = write_inputs(tmp_path, fr.golden_inputs()[case])
    for win in ("64", "4096", ""):
        rc, out, err = run([BINARY], tmp_path, words, env={"PALACE_FILTERRES_WINDOW": win, "PALACE_NO_FORK": "1"})
        assert (rc, err) == (0, b""), err[-600:]
        compare(tmp_path, case, golden, out)
        for o in OUTPUTS:
            (tmp_path / o).unlink()


def fails_with(d, words, message):
    rc, out, err = run([BINARY], d, words)
    assert rc == 1 and out == b"" and err == b"filter_result: " + message + b"\n", (rc, out, err)
    assert not any((d / o).exists() or (d / (o + ".tmp")).exists() for o in OUTPUTS)


@pytest.mark.parametrize("which", ["missing", "blast", "scores", "paths", "fasta", "usage"])
def test_declared_faults(which, tmp_path):
    k = 0

    def fresh(case, missing=None):
        nonlocal k
        k += 1
        d = tmp_path / str(k)
        d.mkdir()
        return d, write_inputs(d, case, missing)
    good = fr.golden_inputs()["headers_first"]
    if which == "missing":
        for key, fn in FILES.items():
            fails_with(*fresh(good, missing=key), b"cannot open " + fn.encode())
    elif which == "fasta":           # two records of one name (the second one's header line is named), text before the first '>'
        fasta = good[0]
        name = fasta[1:fasta.index(b"\n")].split(b" ")[0]
        dup = fasta + b">other\nACG\n>" + name + b" again\nTT\n"
        fails_with(*fresh((dup,) + good[1:]), b"asm.fasta: line %d: sequence name '%s' appears a second time" % (dup.count(b"\n") - 1, name))
        fails_with(*fresh((b"ACGT\n" + fasta,) + good[1:]), b"asm.fasta: line 1: text before the first '>'")
    elif which == "usage":
        d, words = fresh(good)
        for bad in (words[:-1], words + ["x"], words[:4] + ["1e"] + words[5:], words[:4] + ["+0.75"] + words[5:]):
            rc, out, err = run([BINARY], d, bad)
            assert rc == 2 and out == b"" and err.startswith(b"usage: filter_result"), (bad, rc, err)
    else:
        mine = {name: v for name, v in fr.faulty_inputs().items() if v[0] == which}
        assert len(mine) >= 2
        for name, (_, case, line, reason) in mine.items():
            fails_with(*fresh(case), FILES[which].encode() + b": line %d: " % line + reason)
