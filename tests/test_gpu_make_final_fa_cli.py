"""bin/make_final_fa and scripts/make_final_fa.py: every case of tests/golden/final_fa_cases.npz (what the reference's script
itself wrote; PINNED: graph rules, cycle decision, order, numbering, separators, headers, stderr; UNPINNED: the FASTA reader and the
complement table, a stand-in's where the golden file is made) through the executable and through the script, the options in both
spellings, the output window, and the declared faults."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import final_fa_cases as fc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "palace_amd", "bin", "make_final_fa")
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "make_final_fa.py")
FILES = ("final.txt", "graph.txt", "asm.fasta")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "final_fa_cases.npz"))


def write_inputs(d, paths, graph, fasta):
    for fn, text in zip(FILES, (paths, graph, fasta)):
        (d / fn).write_bytes(text)


def run(cmd, d, args, env=None):
    p = subprocess.run(cmd + list(FILES) + ["out.fasta"] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, **(env or {})))
    return p.returncode, p.stdout, p.stderr


@pytest.mark.parametrize("how", ["binary", "script"])
def test_every_golden_case(how, golden, tmp_path):
    cmd = [BINARY] if how == "binary" else [sys.executable, SCRIPT]
    for name, (paths, graph, fasta, prefix, words) in fc.golden_inputs().items():
        d = tmp_path / name
        d.mkdir()
        write_inputs(d, paths, graph, fasta)
        rc, out, err = run(cmd, d, [prefix.decode()] + [w.decode() for w in words])
        assert (rc, out) == (0, b"") and err == golden[name + "__err"].tobytes(), (name, rc, out, err[-600:])
        assert (d / "out.fasta").read_bytes() == golden[name + "__out"].tobytes(), name
        assert not (d / "out.fasta.tmp").exists()


def test_options_in_both_spellings_and_anywhere(golden, tmp_path):
    paths, graph, fasta, prefix, _ = fc.golden_inputs()["random_2"]
    write_inputs(tmp_path, paths, graph, fasta)
    want = fc.final_fa(paths, graph, fasta, prefix, b"asm.fasta", b"out.fasta", 1000, 300)
    assert want[0] == golden["random_2__out"].tobytes()
    for before, after in ((["--trim_threshold", "1000", "--min_cycle_length=300"], []), (["--min_cycle_length", "300"], ["--trim_threshold=1000"]),
                          ([], ["--trim_threshold=1000", "--min_cycle_length", "300"])):
        p = subprocess.run([BINARY] + before + list(FILES) + ["out.fasta", prefix.decode()] + after, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert (p.returncode, p.stdout, p.stderr) == (0, b"", want[1]), p.stderr[-600:]
        assert (tmp_path / "out.fasta").read_bytes() == want[0]
        (tmp_path / "out.fasta").unlink()
    assert fc.final_fa(paths, graph, fasta, prefix, b"asm.fasta", b"out.fasta")[0] != want[0]          # (the options matter on this case)
    for bad in (["--trim", "1000"], ["--trim_threshold"], ["--trim_threshold=x"], ["--min_cycle_length", "1e4"], ["--verbose"], ["extra"]):
        rc, out, err = run([BINARY], tmp_path, [prefix.decode()] + bad)
        assert rc == 2 and out == b"" and err.startswith(b"usage: make_final_fa"), (bad, rc, err)
        assert not (tmp_path / "out.fasta").exists()


@pytest.mark.parametrize("case", ["hand", "random_1"])
def test_the_output_window_does_not_show(case, golden, tmp_path):
    paths, graph, fasta, prefix, words = fc.golden_inputs()[case]
    write_inputs(tmp_path, paths, graph, fasta)
    for win in ("64", "1", "1000000000000"):
        rc, out, err = run([BINARY], tmp_path, [prefix.decode()] + [w.decode() for w in words], env={"PALACE_FINALFA_WINDOW": win, "PALACE_NO_FORK": "1"})
        assert (rc, out) == (0, b"") and err == golden[case + "__err"].tobytes(), err[-600:]
        assert (tmp_path / "out.fasta").read_bytes() == golden[case + "__out"].tobytes(), win


def fails_with(d, message):
    rc, out, err = run([BINARY], d, ["P"])
    assert rc == 1 and out == b"" and err == b"make_final_fa: " + message + b"\n", (rc, err)
    assert not (d / "out.fasta").exists() and not (d / "out.fasta.tmp").exists()


def test_declared_faults(tmp_path):
    paths, graph, fasta, _, _ = fc.golden_inputs()["hand"]
    k = 0

    def fresh(p=paths, g=graph, f=fasta, missing=None):
        nonlocal k
        k += 1
        d = tmp_path / str(k)
        d.mkdir()
        write_inputs(d, p, g, f)
        if missing:
            (d / missing).unlink()
        return d
    for fn in FILES:
        fails_with(fresh(missing=fn), b"cannot open " + fn.encode())
    faulty = fc.faulty_inputs()
    for name in ("paths_no_length", "paths_high_byte", "paths_two_faults", "graph_bad_orientation", "graph_high_byte_in_comment", "graph_no_length"):
        which, text, line, reason = faulty[name]
        d = fresh(p=text) if which == "paths" else fresh(g=text)
        fails_with(d, (b"final.txt" if which == "paths" else b"graph.txt") + b": line %d: " % line + reason)
    # two records of one name: the second one's header line is named
    name = fasta[1:fasta.index(b"\n")].split(b" ")[0]
    dup = fasta + b">other_length_3\nACG\n>" + name + b" again\nTT\n"
    fails_with(fresh(f=dup), b"asm.fasta: line %d: sequence name '%s' appears a second time" % (dup.count(b"\n") - 1, name))
    # the FASTA's own faults as make_fa_from_path words them
    fails_with(fresh(f=b"ACGT\n" + fasta), b"asm.fasta: line 1: text before the first '>'")
    fails_with(fresh(f=fasta + b">x_length_1\nAC\xe9T\n"), b"asm.fasta: line %d: a sequence byte outside 0x21-0x7E" % (fasta.count(b"\n") + 2))
