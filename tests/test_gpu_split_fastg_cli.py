"""bin/split_fastg and scripts/split_fastg.py on a GPU: files in, files out, stderr and exit status against what the reference's
script wrote (tests/golden/split_fastg_cases.npz) and the Python restatement of tests/split_fastg_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import path_fasta_cases as pc
from tests import split_fastg_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "palace_amd", "bin", "split_fastg")
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "split_fastg.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_fastg_cases.npz")


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def files(tmp_path_factory, golden):
    d = tmp_path_factory.mktemp("split_fastg")
    (d / "assembly_graph.fastg").write_bytes(golden["spades60__in"].tobytes())
    return d


def read(p):
    return p.read_bytes() if p.exists() else None


def test_binary_and_script_write_the_reference_bytes(files, golden):
    want = golden["spades60__out"].tobytes()
    g = str(files / "assembly_graph.fastg")
    p = run([TOOL, "-g", g, "-o", str(files / "bin.fasta")])
    q = run([sys.executable, SCRIPT, "--graph=" + g, "--output", str(files / "script.fasta")])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"") == (q.returncode, q.stdout, q.stderr)
    assert read(files / "bin.fasta") == want == read(files / "script.fasta")
    assert not (files / "bin.fasta.fai").exists() and not (files / "assembly_graph.fastg.fai").exists()


def test_default_output_name(files, golden):
    p = run([TOOL, "--graph", str(files / "assembly_graph.fastg")])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
    assert read(files / "assembly_graph.nodes.fasta") == golden["spades60__out"].tobytes()


def test_trace_goes_to_stderr(files):
    p = run([TOOL, "-g", str(files / "assembly_graph.fastg"), "-o", str(files / "traced.fasta")], env=dict(os.environ, PALACE_TRACE="1", PALACE_NO_FORK="1"))
    assert p.returncode == 0 and p.stdout == b"" and b"[split_fastg] output written" in p.stderr


def test_fai_files(tmp_path, golden):
    text = golden["spades70_crlf__in"].tobytes() + golden["empty_sequences__in"].tobytes().replace(b"E_", b"F_")
    g, o = tmp_path / "assembly_graph.fastg", tmp_path / "assembly_graph.fasta"
    g.write_bytes(text)
    p = run([TOOL, "-g", str(g), "-o=" + str(o), "--fai"])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
    fasta = read(o)
    assert fasta == sc.split_fastg(text)
    assert read(tmp_path / "assembly_graph.fasta.fai") == sc.output_fai(text)
    assert read(tmp_path / "assembly_graph.fastg.fai") == sc.graph_fai(text)[0]
    # the FASTA's rows against an index of the written FASTA (a record without bases: the line fields are 0 here by rule)
    recs, code, _ = pc.fasta_index(fasta)
    assert code == pc.OK
    rows = [l.split(b"\t") for l in read(tmp_path / "assembly_graph.fasta.fai").split(b"\n")[:-1]]
    assert len(rows) == len(recs) >= 10
    for row, r in zip(rows, recs):
        assert (row[0], int(row[1]), int(row[2])) == (r["name"], r["length"], r["seq_off"])
        assert (int(row[3]), int(row[4])) == ((r["line_bases"], r["line_width"]) if r["length"] else (0, 0))
        assert pc.sequence_of(fasta, dict(r, line_bases=int(row[3]), line_width=int(row[4]))) == fasta[r["seq_off"]:r["seq_off"] + r["length"]]


def test_duplicate_whole_header_is_left_out_with_a_warning(tmp_path):
    text = b">E_1:E_2;\nACGT\n>E_2;\nAC\n>E_1:E_2;\nGG\n>E_1:E_3; x\nTT\n"
    g = tmp_path / "dup.fastg"
    g.write_bytes(text)
    p = run([TOOL, "-g", str(g), "--fai"])
    assert p.returncode == 0 and p.stdout == b""
    assert p.stderr.count(b"\n") == 1 and b"warning" in p.stderr and b"'E_1:E_2;'" in p.stderr and b"record 3" in p.stderr
    assert read(tmp_path / "dup.nodes.fasta") == b">E_1\nACGT\n>E_2\nAC\n" == sc.split_fastg(text)
    rows, left_out = sc.graph_fai(text)
    assert left_out == [b"E_1:E_2;"] and read(tmp_path / "dup.fastg.fai") == rows == b"E_1:E_2;\t4\t10\t4\t5\nE_2;\t2\t21\t2\t3\nE_1:E_3;\t2\t49\t2\t3\n"
    assert read(tmp_path / "dup.nodes.fasta.fai") == b"E_1\t4\t5\t4\t5\nE_2\t2\t15\t2\t3\n"


@pytest.mark.parametrize("name", sorted(sc.fault_cases()))
def test_errors_exit_1_and_leave_an_empty_output(tmp_path, name):
    text, code, line = sc.fault_cases()[name]
    g, o = tmp_path / "bad.fastg", tmp_path / "out.fasta"
    g.write_bytes(text)
    p = run([TOOL, "-g", str(g), "-o", str(o), "--fai"])
    assert p.returncode == 1 and p.stdout == b"" and read(o) == b""
    assert b"bad.fastg" in p.stderr and b"line %d:" % line in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
    assert not (tmp_path / "out.fasta.fai").exists() and not (tmp_path / "bad.fastg.fai").exists()
    if name in ("no_final_lf", "two_faults"):
        q = run([sys.executable, SCRIPT, "-g", str(g), "-o", str(tmp_path / "script.fasta")])
        assert (q.returncode, q.stdout, read(tmp_path / "script.fasta")) == (1, b"", b"")
        assert q.stderr.replace(b"script.fasta", b"out.fasta") == p.stderr


def test_missing_graph(tmp_path):
    p = run([TOOL, "-g", str(tmp_path / "nowhere.fastg"), "-o", str(tmp_path / "o.fasta")])
    assert p.returncode == 1 and b"cannot open" in p.stderr and not (tmp_path / "o.fasta").exists()


@pytest.mark.parametrize("argv", [[], ["-o", "x.fasta"], ["-g"], ["-g", "graph.txt"], ["-g", "a.fastg", "--nope"], ["-g", "a.fastg", "stray"],
                                  ["-g", "dir/.fastg"]])
def test_usage_errors_exit_2(tmp_path, argv):
    for cmd in ([TOOL], [sys.executable, SCRIPT]):
        p = run(cmd + argv, cwd=tmp_path)
        assert p.returncode == 2 and p.stdout == b"" and b"usage" in p.stderr
    assert not list(tmp_path.iterdir())
