"""bin/make_fa_from_path and scripts/make_fa_from_path.py on a GPU: files in, files out, stdout, stderr and exit status against
the Python restatement of tests/path_fasta_cases.py (the reference's script needs pysam, which is absent: parity is unpinned)."""
import os
import subprocess
import sys

import pytest

from palace_amd import synth
from tests import graph_cases as gc
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOL = os.path.join(BIN, "make_fa_from_path")
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "make_fa_from_path.py")


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("make_fa")
    fasta, _ = pc.chain_fasta(synth.rng_for(31))
    (d / "asm.fa").write_bytes(fasta)
    (d / "paths.txt").write_bytes(pc.CHAIN_PATHS)
    return d, fasta


def tool(d, paths_name, out_name, mode, cmd=(TOOL,), env=None):
    out = d / out_name
    p = run([*cmd, str(d / "asm.fa"), str(d / paths_name), str(out), mode], env=env)
    return p, out.read_bytes() if out.exists() else None


@pytest.mark.parametrize("mode", ["0", "1", "name"])
def test_modes(files, mode):
    d, fasta = files
    want, want_stdout = pc.make_fa(fasta, pc.CHAIN_PATHS, mode.encode())
    p, got = tool(d, "paths.txt", f"out_{mode}.fa", mode)
    assert p.returncode == 0 and p.stderr.count(b"\n") == 1 and b"NODE_6" in p.stderr, p.stderr     # (the duplicate name's warning)
    assert got == want
    assert p.stdout == want_stdout == b"make_fa_from_path.py running\nContig not found: plain\n"
    if mode == "0":
        # iter / self / blank lines count in the numbering; an empty sequence keeps both of its lines; no LF at the file's end
        assert [l for l in got.split(b"\n") if l.startswith(b">")] == [b">res_%d_%d" % (i, n) for i, n in
                                                                      ((1, 5060), (3, 5121), (6, 42), (7, 199), (8, 74), (10, 0), (11, 77))]
        assert b">res_10_0\n\n>res_11_77\n" in got
    else:
        assert b">x+-x+NODE_1+N ODE_ 4+\n" in got and b">NODE_6+NODE_6-\n" in got      # TABs gone, the spaces inside a token kept


def test_small_windows_write_the_same_bytes(files):
    d, fasta = files
    want, _ = pc.make_fa(fasta, pc.CHAIN_PATHS, b"0")
    for w in ("64", "1000", "4097"):
        p, got = tool(d, "paths.txt", f"out_w{w}.fa", "0", env=dict(os.environ, PALACE_PATHFA_WINDOW=w))
        assert p.returncode == 0 and got == want, (w, p.stderr)


def test_missing_contig(files):
    d, fasta = files
    (d / "missing.txt").write_bytes(b"NODE_1+\tplain_7\niter 1\nNODE_2+\tgone_1\tNODE_3_x_y+\nNODE_1+\n")
    p, got = tool(d, "missing.txt", "missing.fa", "0")
    assert p.returncode == 1 and got == b""
    assert p.stdout == b"make_fa_from_path.py running\nContig not found: plain\nContig not found: gone\n"
    err = [l for l in p.stderr.split(b"\n") if l and b"warning" not in l]
    assert len(err) == 1 and b"missing.txt" in err[0] and b"line 3" in err[0] and b"'gone_1'" in err[0]
    try:
        pc.make_fa(fasta, (d / "missing.txt").read_bytes(), b"0")
        raise AssertionError("the restatement must fail too")
    except pc.MissingContig as m:
        assert (m.line, m.token, m.stdout) == (3, b"gone_1", p.stdout)


@pytest.mark.parametrize("case", sorted(pc.malformed_fastas(synth.rng_for(4))))
def test_malformed_fasta(tmp_path, case):
    text, code, line = pc.malformed_fastas(synth.rng_for(4))[case]
    (tmp_path / "asm.fa").write_bytes(text)
    (tmp_path / "p.txt").write_bytes(b"r0+\n")
    p, got = tool(tmp_path, "p.txt", "out.fa", "0")
    assert p.returncode == 1 and got is None                                          # nothing is written, not even an empty file
    assert b"asm.fa" in p.stderr and b"line %d:" % line in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
    assert p.stdout == b"make_fa_from_path.py running\n"


def test_batch_equals_separate_runs(files):
    d, fasta = files
    lists = {"b0.txt": pc.CHAIN_PATHS, "b1.txt": b"NODE_5-\nNODE_1+\tNODE_2-\n", "b2.txt": b"iter 0\n"}
    modes = {"b0.txt": "1", "b1.txt": "0", "b2.txt": "0"}
    for name, text in lists.items():
        (d / name).write_bytes(text)
    (d / "batch.lst").write_text("".join(f"{d / n}  {d / (n + '.batch.fa')}\t{modes[n]}\n" for n in lists) + "\n")
    p = run([TOOL, "--batch", str(d / "batch.lst"), str(d / "asm.fa")])
    assert p.returncode == 0, p.stderr
    stdout = b""
    for n in lists:
        q, got = tool(d, n, n + ".single.fa", modes[n])
        assert q.returncode == 0 and got == (d / (n + ".batch.fa")).read_bytes() == pc.make_fa(fasta, lists[n], modes[n].encode())[0]
        stdout += q.stdout
    assert p.stdout == stdout and (d / "b2.txt.batch.fa").read_bytes() == b""


def test_batch_with_a_failing_entry(files):
    d, fasta = files
    (d / "ok.txt").write_bytes(b"NODE_5+\tNODE_3-\n")
    (d / "bad.txt").write_bytes(b"NODE_1+\nnot_there+\n")
    (d / "fail.lst").write_text(f"{d / 'ok.txt'} {d / 'f0.fa'} 0\n{d / 'bad.txt'} {d / 'f1.fa'} 0\n{d / 'ok.txt'} {d / 'f2.fa'} 0\n")
    p = run([TOOL, "--batch", str(d / "fail.lst"), str(d / "asm.fa")])
    assert p.returncode == 1 and b"bad.txt" in p.stderr and b"line 2" in p.stderr
    assert (d / "f0.fa").read_bytes() == pc.make_fa(fasta, b"NODE_5+\tNODE_3-\n", b"0")[0]
    assert (d / "f1.fa").read_bytes() == b"" and not (d / "f2.fa").exists()


def test_script_is_the_binary(files):
    d, fasta = files
    p, got = tool(d, "paths.txt", "bin.fa", "0")
    q, got_s = tool(d, "paths.txt", "script.fa", "0", cmd=(sys.executable, SCRIPT))
    assert (q.returncode, q.stdout, q.stderr, got_s) == (p.returncode, p.stdout, p.stderr, got)
    p, got = tool(d, "missing.txt", "bin_missing.fa", "0")
    q, got_s = tool(d, "missing.txt", "script_missing.fa", "0", cmd=(sys.executable, SCRIPT))
    assert q.returncode == p.returncode == 1 and q.stdout == p.stdout and got_s == got == b""
    assert q.stderr.replace(b"script_missing", b"bin_missing") == p.stderr
    q = run([sys.executable, SCRIPT, "only", "three", "arguments"])
    assert q.returncode == 1 and b"Usage" in q.stderr


def test_matching_to_sequences(tmp_path):
    """a graph of tests/graph_cases.py through bin/matching, the cycles through scripts/remove_cycle_dup.py, both result files
    through the tool: what the restatement makes of the same files"""
    rng = synth.rng_for(32)
    fasta = pc.fasta_text([(nm.encode() + b" len=%d" % n, pc.random_seq(rng, n)) for nm, n in gc.TARGETS], 60)
    g, lin, cyc, dedup = (str(tmp_path / n) for n in ("graph.txt", "linear.txt", "cycle.txt", "cycle_dedup.txt"))
    (tmp_path / "asm.fa").write_bytes(fasta)
    open(g, "wb").write(gc.EXPECTED)
    r = run([os.path.join(BIN, "matching"), "-g", g, "-r", lin, "-c", cyc, "-i", "10", "-b", "--aggressive"])
    assert r.returncode == 0, r.stderr
    r = run([sys.executable, os.path.join(ROOT, "palace_amd", "scripts", "remove_cycle_dup.py"), cyc, dedup])
    assert r.returncode == 0, r.stderr
    records = 0
    for name in ("linear.txt", "cycle_dedup.txt"):
        paths = (tmp_path / name).read_bytes()
        want, want_stdout = pc.make_fa(fasta, paths, b"0")
        p, got = tool(tmp_path, name, name + ".fa", "0")
        assert p.returncode == 0 and p.stderr == b"" and p.stdout == want_stdout and got == want
        records += want.count(b">")
    assert records >= 1 and b"ctg" in (tmp_path / "linear.txt").read_bytes() + (tmp_path / "cycle_dedup.txt").read_bytes()
