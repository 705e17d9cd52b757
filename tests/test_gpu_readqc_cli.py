"""bin/readqc on a GPU: files in, files out, the JSON report, stderr and exit status against the Python restatement of
tests/readqc_cases.py (fastp is absent: parity is unpinned).  The sample is a synthetic FASTQ pair whose short fragments are read
through into the adapters."""
import json
import os
import subprocess

import numpy as np
import pytest

from palace_amd import synth
from tests import gz_util
from tests import readqc_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOL = os.path.join(BIN, "readqc")
ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")       # Illumina TruSeq, as published
READ = 150


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def sample(rng, template: np.ndarray, n_pairs: int):
    """pairs of 150 bases from fragments of 20 .. 400 bases of `template`: a fragment shorter than a read runs into the adapter and
    random bases behind it; 0.5 % substitutions, a few N, and quality tails that fall off"""
    recs1, recs2 = [], []
    for i in range(n_pairs):
        ins = int(np.clip(rng.normal(170, 70), 20, 400))
        st = int(rng.integers(0, len(template) - ins))
        frag = template[st:st + ins]
        reads = []
        for k, piece in enumerate((frag, synth.revcomp(frag))):
            tail = np.frombuffer(ADAPTERS[k] + rc.random_seq(rng, READ), np.uint8)
            s = synth.mutate(rng, np.concatenate([piece, tail])[:READ], 0.005)
            if rng.random() < 0.03:
                s[rng.integers(0, READ, size=int(rng.integers(1, 10)))] = ord("N")
            qual = np.full(READ, 33 + 37, np.uint8)
            if rng.random() < 0.25:
                qual[int(rng.integers(0, READ)):] = 33 + 2
            reads.append((s.tobytes(), qual.tobytes()))
        recs1.append((b"r%d/1" % i, *reads[0]))
        recs2.append((b"r%d/2" % i, *reads[1]))
    return rc.fastq(recs1), rc.fastq(recs2)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("readqc")
    rng = synth.rng_for(58)
    db = synth.make_phage_db(rng, 3, 4000, 6000)
    db.write_fasta(str(d / "db.fa"))
    t1, t2 = sample(rng, np.concatenate(db.seqs), 3000)
    (d / "r_1.fq").write_bytes(t1)
    (d / "r_2.fq").write_bytes(t2)
    want = rc.readqc(t1, t2)
    assert want["trimmed_reads"] > 1000 and want["low_quality"] > 50 and want["too_many_n"] > 10 and want["reads_after"] > 3000
    (d / "want_1.fq").write_bytes(want["out1"])
    (d / "want_2.fq").write_bytes(want["out2"])
    return d, t1, t2, want


def tool(d, tag, in1="r_1.fq", in2="r_2.fq", extra=(), env=None, report=True):
    o1, o2, js, html = (d / f"{tag}_1.fq", d / f"{tag}_2.fq", d / f"{tag}.json", d / f"{tag}.html")
    cmd = [TOOL, "-i", str(d / in1), "-I", str(d / in2), "-o", str(o1), "-O", str(o2), "-w", "8"] + (["-j", str(js), "-h", str(html)] if report else [])
    p = run(cmd + list(extra), env=env)
    return p, [f.read_bytes() if f.exists() else None for f in (o1, o2, js, html)]


def nothing_left(d, tag):
    return [p.name for p in d.iterdir() if p.name.startswith(tag)] == []


def test_files_and_report_equal_the_restatement(files):
    d, _, _, want = files
    p, (o1, o2, js, html) = tool(d, "plain")
    assert p.returncode == 0 and p.stdout == b"" and p.stderr == b"", p.stderr
    assert o1 == want["out1"] and o2 == want["out2"]
    assert json.loads(js) == rc.report(want)
    assert html.count(b"\n") == 1 and b"plain.json" in html
    assert nothing_left(d, "plain_1.fq.tmp") and nothing_left(d, "plain_2.fq.tmp")
    p, (o1, o2, js, html) = tool(d, "bare", report=False)                   # -j and -h are optional
    assert p.returncode == 0 and (o1, o2, js, html) == (want["out1"], want["out2"], None, None)


def test_options(files):
    d, t1, t2, _ = files
    for tag, extra, kw in (("A", ["-A"], {"no_trim": 1}), ("QL", ["--disable_quality_filtering", "-L"], {"no_quality_filter": 1, "no_length_filter": 1}),
                           ("num", ["-q", "20", "--unqualified_percent_limit=30", "-n", "2", "--length_required", "60"],
                            {"qualified_quality": 20, "unqualified_percent": 30, "n_limit": 2, "min_length": 60})):
        want = rc.readqc(t1, t2, rc.params(**kw))
        p, (o1, o2, js, _) = tool(d, "opt" + tag, extra=extra)
        assert p.returncode == 0 and p.stderr == b"", (tag, p.stderr)
        assert o1 == want["out1"] and o2 == want["out2"] and json.loads(js) == rc.report(want), tag


def test_compressed_inputs_give_the_same_bytes(files):
    d, t1, t2, want = files
    forms = {"gzip": (gz_util.gzip_member(t1), gz_util.gzip_member(t2, fname=b"r_2.fq")), "bgzf": (gz_util.bgzf(t1), gz_util.bgzf(t2, block=4000)),
             "mixed": (gz_util.gzip_members(t1, [1000, len(t1) // 2]), t2), "stored": (t1, gz_util.bgzf(t2, level=0))}
    for tag, (a, b) in forms.items():
        (d / f"{tag}_in_1.fq.gz").write_bytes(a)
        (d / f"{tag}_in_2.fq.gz").write_bytes(b)
        p, (o1, o2, js, _) = tool(d, tag, in1=f"{tag}_in_1.fq.gz", in2=f"{tag}_in_2.fq.gz")
        assert p.returncode == 0 and p.stderr == b"", (tag, p.stderr)
        assert o1 == want["out1"] and o2 == want["out2"] and json.loads(js) == rc.report(want), tag


def test_damaged_gzip(files):
    d, t1, t2, _ = files
    whole = gz_util.gzip_member(t2)
    damaged = bytearray(whole)
    damaged[len(whole) // 2] ^= 0x5a
    for tag, blob in (("cut", whole[:len(whole) * 2 // 3]), ("cut_trailer", whole[:-3]), ("flip", bytes(damaged)), ("tail", whole + b"junk")):
        (d / f"{tag}_in_2.fq.gz").write_bytes(blob)
        p, outs = tool(d, "gz" + tag, in2=f"{tag}_in_2.fq.gz")
        assert p.returncode == 1 and p.stdout == b"" and outs == [None] * 4, (tag, p.stderr)
        assert p.stderr.startswith(b"readqc: ") and b"_in_2.fq.gz: zlib: " in p.stderr and p.stderr.count(b"\n") == 1, (tag, p.stderr)
        assert nothing_left(d, "gz" + tag)


def test_small_windows_write_the_same_files(files):
    d, _, _, want = files
    one_record = int(want["off1"][want["off1"] > 0][0])
    for w in (1 << 20, one_record, 4097):
        p, (o1, o2, _, _) = tool(d, f"win{w}", env=dict(os.environ, PALACE_READQC_WINDOW=str(w)))
        assert p.returncode == 0 and o1 == want["out1"] and o2 == want["out2"], (w, p.stderr)


def test_eref_reads_the_outputs_as_it_reads_the_restatements(files):
    d, _, _, want = files
    p, _ = tool(d, "foreref")
    assert p.returncode == 0
    outs = []
    for a, b in (("foreref_1.fq", "foreref_2.fq"), ("want_1.fq", "want_2.fq")):
        e = run([os.path.join(BIN, "eref"), str(d / a), str(d / b), str(d / "db.fa"), str(d / "eref_tmp.txt"), "0.9", "0.85", "4"])
        assert e.returncode == 0, e.stderr
        outs.append(e.stdout)
    assert outs[0] == outs[1] and outs[0] != b""


def test_faults_leave_nothing_behind(files):
    d, t1, t2, _ = files
    lines1, lines2 = t1.split(b"\n"), t2.split(b"\n")
    bad1 = b"\n".join(lines1[:401] + [lines1[401].replace(b"A", b"a", 1)] + lines1[402:])           # line 402 of file 1: a base
    bad2 = b"\n".join(lines2[:43] + [lines2[43][:-1]] + lines2[44:])                                # line 44 of file 2: QUAL one short
    short2 = b"\n".join(lines2[:-5]) + b"\n"                                                        # file 2 one record short
    for name, text in (("bad_1.fq", bad1), ("bad_2.fq", bad2), ("short_2.fq", short2), ("cr_2.fq", t2.replace(b"\n", b"\r\n"))):
        (d / name).write_bytes(text)
    for tag, in1, in2, msg in (("f1", "bad_1.fq", "r_2.fq", b"bad_1.fq: line 402: a base other than"), ("f2", "r_1.fq", "bad_2.fq", b"bad_2.fq: line 44: the quality line"),
                               ("f12", "bad_1.fq", "bad_2.fq", b"bad_1.fq: line 402: "), ("f2cr", "r_1.fq", "cr_2.fq", b"cr_2.fq: line 2: a base other than"),
                               ("count", "r_1.fq", "short_2.fq", b"short_2.fq: 2999 records, but"), ("count_after_fault", "r_1.fq", "bad_2.fq", b"bad_2.fq: line 44: "),
                               ("missing", "r_1.fq", "nowhere.fq", b"cannot open")):
        p, outs = tool(d, tag, in1=in1, in2=in2)
        assert p.returncode == 1 and p.stdout == b"" and outs == [None] * 4, (tag, p.stderr)
        assert p.stderr.startswith(b"readqc: ") and msg in p.stderr and p.stderr.count(b"\n") == 1, (tag, p.stderr)
        assert nothing_left(d, tag)
    assert rc.verdict(bad1)[1:] == (402, rc.EBASE) and rc.verdict(bad2)[1:] == (44, rc.EQLEN) and rc.verdict(short2) == (2999, 0, 0)
