"""bin/faidx on a GPU: files in, files out, stdout, stderr and exit status against the Python restatement of tests/faidx_cases.py
(parity with `samtools faidx` is UNPINNED: samtools is absent; tests/test_host_faidx_rules.py pins the restatement to a hand-typed
catalogue), and its index against the one `split_fastg --fai` writes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from tests import faidx_cases as fx
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "palace_amd", "bin", "faidx")
SPLIT = os.path.join(ROOT, "palace_amd", "bin", "split_fastg")
GOLDEN = os.path.join(ROOT, "tests", "golden", "split_fastg_cases.npz")


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def read(p):
    return p.read_bytes() if p.exists() else None


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """a FASTA of 400 records in lines of 60, and regions of every kind that succeeds"""
    rng = np.random.default_rng(5)
    text, names = fx.synthetic_assembly(rng, 400, max_len=700)
    d = tmp_path_factory.mktemp("faidx")
    (d / "assembly.fasta").write_bytes(text)
    regions = []
    for i in rng.integers(0, len(names), size=240):
        b, e = sorted(int(x) for x in rng.integers(1, 500, size=2))
        regions.append((names[i], names[i] + b":%d-%d" % (b, e), names[i] + b":%d-" % b, names[i] + b":-%d" % e, names[i] + b":0,%03d-" % b)[int(rng.integers(0, 5))])
    return d, text, names, regions


def test_index_mode_writes_the_rows_of_split_fastg_and_of_the_restatement(tmp_path):
    text = np.load(GOLDEN)["spades60__in"].tobytes()
    (tmp_path / "a.fastg").write_bytes(text)
    (tmp_path / "b.fasta").write_bytes(text)
    p = run([SPLIT, "-g", str(tmp_path / "a.fastg"), "--fai"])
    q = run([TOOL, str(tmp_path / "b.fasta")])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"") == (q.returncode, q.stdout, q.stderr)
    rows, dropped = fx.fai_rows(text)
    assert dropped == [] and rows.count(b"\n") > 10
    assert read(tmp_path / "b.fasta.fai") == rows == read(tmp_path / "a.fastg.fai")
    assert not (tmp_path / "b.fasta.fai.tmp").exists()


def test_index_mode_warns_about_a_name_that_appears_again(tmp_path):
    f = tmp_path / "dup.fa"
    f.write_bytes(fx.CATALOGUE_FASTA)
    p = run([TOOL, str(f)])
    assert p.returncode == 0 and p.stdout == b""
    assert p.stderr == b"faidx: warning: %s: sequence name 'chr1' appears again in record 4: left out of %s.fai\n" % (str(f).encode(), str(f).encode())
    assert read(tmp_path / "dup.fa.fai") == fx.fai_rows(fx.CATALOGUE_FASTA)[0]


def test_index_mode_on_a_ragged_text_leaves_the_index_as_it_was(tmp_path):
    text, code, line = pc.malformed_fastas(np.random.default_rng(3))["ragged_middle"]
    f = tmp_path / "ragged.fa"
    f.write_bytes(text)
    (tmp_path / "ragged.fa.fai").write_bytes(b"an older index\n")
    p = run([TOOL, str(f)])
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"faidx: %s: line %d: %s\n" % (str(f).encode(), line, fx.FAULT_TEXT[code])
    assert read(tmp_path / "ragged.fa.fai") == b"an older index\n" and not (tmp_path / "ragged.fa.fai.tmp").exists()


def test_fetch_gives_the_same_bytes_whatever_the_way(assembly):
    d, text, names, regions = assembly
    fa = str(d / "assembly.fasta")
    want, err, status = fx.fetch(text, regions)
    assert status == 0 and want.count(b">") == len(regions) and len(want) > 20000
    p = run([TOOL, fa] + [r.decode() for r in regions], env=dict(os.environ, PALACE_FAIDX_WINDOW="64"))
    assert (p.returncode, p.stderr) == (0, err) and p.stdout == want
    (d / "regions.txt").write_bytes(b"\r\n".join(regions) + b"\r\n")
    p = run([TOOL, "--output", str(d / "from_file.fa"), "-r", str(d / "regions.txt"), fa])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", err) and read(d / "from_file.fa") == want
    (d / "half.txt").write_bytes(b"\n".join(regions[:100]))                     # (no LF at the end)
    p = run([TOOL, "-o", str(d / "both.fa"), "--region-file=" + str(d / "half.txt"), fa] + [r.decode() for r in regions[100:]])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", err) and read(d / "both.fa") == want
    assert not (d / "assembly.fasta.fai").exists() and not (d / "both.fa.tmp").exists()


@pytest.mark.parametrize("keep_going", [False, True], ids=["stop", "continue"])
def test_a_failing_region(assembly, tmp_path, keep_going):
    d, text, names, regions = assembly
    mine = [regions[0], b"NODE_0:7-3", regions[1], b"", names[1] + b":9999", b"nowhere"]
    (tmp_path / "r.txt").write_bytes(b"\n".join(mine[:4]) + b"\n")                 # a blank line is a region, and fails
    want, err, status = fx.fetch(text, mine, n=13, keep_going=keep_going)
    assert status == (0 if keep_going else 1) and err.count(b"Failed") == (3 if keep_going else 1)
    assert (b"[faidx] Zero length sequence: " + names[1] + b":9999\n" in err) == keep_going
    out = tmp_path / "out.fa"
    p = run([TOOL, "-n", "13", "-r", str(tmp_path / "r.txt"), "-o", str(out)] + (["-c"] if keep_going else []) + [str(d / "assembly.fasta"), (names[1] + b":9999").decode(), "nowhere"])
    assert (p.returncode, p.stdout, p.stderr) == (status, b"", err)
    assert read(out) == (want if keep_going else None) and not (tmp_path / "out.fa.tmp").exists()
    if not keep_going:
        assert err == b"[faidx] Failed to fetch sequence in NODE_0:7-3\n"


@pytest.mark.parametrize("mark", ["rc", "sign", "no"])
def test_the_other_strand_with_each_mark(tmp_path, mark):
    f = tmp_path / "c.fa"
    f.write_bytes(fx.CATALOGUE_FASTA)
    regions = [b"ambi", b"chr1:3-12", b"p|q|r", b"ambi:10-13"]
    want, err, _ = fx.fetch(fx.CATALOGUE_FASTA, regions, n=7, reverse=True, mark=mark)
    p = run([TOOL, "-i", "--length", "7", "--mark-strand", mark, str(f)] + [r.decode() for r in regions])
    assert (p.returncode, p.stdout, p.stderr) == (0, want, err)
    assert want.startswith({"rc": b">ambi/rc\n*nacgtN", "sign": b">ambi(-)\n*nacgtN", "no": b">ambi\n*nacgtN"}[mark])


def test_names_out_of_a_paths_fasta_round_trip(tmp_path):
    rng = np.random.default_rng(9)
    records = [(b"res_%d_%d" % (i + 1, n), pc.random_seq(rng, n)) for i, n in enumerate([13, 0, 1, 60, 61, 4000, 120])]
    text = b"".join(b">" + h + b"\n" + s + b"\n" for h, s in records)          # every sequence one line, as make_fa_from_path writes
    f, o = tmp_path / "paths.fa", tmp_path / "picked.fa"
    f.write_bytes(text)
    order = [5, 0, 3, 6, 2, 4]
    p = run([TOOL, str(f), "-o", str(o)] + [records[k][0].decode() for k in order])
    assert (p.returncode, p.stdout, p.stderr) == (0, b"", b"")
    picked = read(o)
    assert picked == fx.fetch(text, [records[k][0] for k in order])[0]
    q = run([TOOL, str(o)])
    assert (q.returncode, q.stdout, q.stderr) == (0, b"", b"")
    assert read(tmp_path / "picked.fa.fai") == fx.fai_rows(picked)[0]
    recs, code, _ = pc.fasta_index(picked)
    assert code == pc.OK and [(r["name"], pc.sequence_of(picked, r)) for r in recs] == [records[k] for k in order]


@pytest.mark.parametrize("argv", [["-f"], ["--fastq"], ["--fai-idx", "x.fai"], ["--gzi-idx=x.gzi"], ["--mark-strand", "custom,<,>"], ["-x"], ["-n", "0"]],
                         ids=lambda a: a[0].lstrip("-") + ("_" + a[1][:6] if len(a) > 1 else ""))
def test_refused_options_exit_2(tmp_path, argv):
    (tmp_path / "a.fa").write_bytes(b">a\nACGT\n")
    p = run([TOOL] + argv + ["a.fa", "a"], cwd=tmp_path)
    assert p.returncode == 2 and p.stdout == b"" and b"usage" in p.stderr
    assert sorted(x.name for x in tmp_path.iterdir()) == ["a.fa"]


def test_a_gzip_input_is_not_read(tmp_path):
    f = tmp_path / "a.fa.gz"
    f.write_bytes(gzip.compress(b">a\nACGT\n"))
    p = run([TOOL, str(f)])
    assert (p.returncode, p.stdout) == (1, b"") and p.stderr == b"faidx: %s: compressed FASTA is not read\n" % str(f).encode()
    assert not (tmp_path / "a.fa.gz.fai").exists()
