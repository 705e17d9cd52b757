"""bin/readqc --full-report on a GPU: the JSON against the restatement's dict of tests/readqc_report_cases.py (`==`, floats included),
the FASTQ outputs against a run without the option, and the option's usage error.  The sample has trimmed, dropped and N-rich pairs,
read 2 longer than read 1, and goes in gzip-compressed too.  (fastp is absent: parity is unpinned.)"""
import json
import os
import subprocess

import numpy as np
import pytest

from palace_amd import capi, synth
from tests import gz_util
from tests import readqc_cases as rc
from tests import readqc_report_cases as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "palace_amd", "bin", "readqc")
ADAPTERS = (b"AGATCGGAAGAGCACACGTCTGAACTCCAGTCA", b"AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT")       # Illumina TruSeq, as published
READ = (140, 151)                                                            # read 2 is the longer one


def sample(rng, n_pairs: int):
    """pairs from fragments of 20 .. 400 bases of one random template; a fragment shorter than a read runs into the adapter; a few
    substitutions, N-rich reads, qualities on both sides of Q20 and Q30 with tails that fall off"""
    template = synth.random_dna(rng, 20000)
    recs = ([], [])
    for i in range(n_pairs):
        ins = int(np.clip(rng.normal(170, 70), 20, 400))
        st = int(rng.integers(0, len(template) - ins))
        frag = template[st:st + ins]
        for k, piece in enumerate((frag, synth.revcomp(frag))):
            tail = np.frombuffer(ADAPTERS[k] + rc.random_seq(rng, READ[k]), np.uint8)
            s = synth.mutate(rng, np.concatenate([piece, tail])[:READ[k]], 0.005)
            if rng.random() < 0.05:
                s[rng.integers(0, READ[k], size=int(rng.integers(1, 12)))] = ord("N")
            qual = rng.choice(np.array([33 + 37, 33 + 37, 33 + 30, 33 + 29, 33 + 20, 33 + 19], np.uint8), size=READ[k])
            if rng.random() < 0.25:
                qual[int(rng.integers(0, READ[k])):] = 33 + 2
            recs[k].append((b"r%d/%d" % (i, k + 1), s.tobytes(), qual.tobytes()))
    return rc.fastq(recs[0]), rc.fastq(recs[1])


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("readqc_report")
    t1, t2 = sample(synth.rng_for(61), 2000)
    (d / "r_1.fq").write_bytes(t1)
    (d / "r_2.fq").write_bytes(t2)
    (d / "r_1.fq.gz").write_bytes(gz_util.gzip_member(t1))
    (d / "r_2.fq.gz").write_bytes(gz_util.bgzf(t2, block=4000))
    want = rc.readqc(t1, t2)
    assert want["trimmed_reads"] > 500 and want["low_quality"] > 50 and want["too_many_n"] > 10 and want["reads_after"] > 2000
    return d, t1, t2, want


def tool(d, tag, extra=(), in1="r_1.fq", in2="r_2.fq", json_out=True):
    o1, o2, js = d / f"{tag}_1.fq", d / f"{tag}_2.fq", d / f"{tag}.json"
    cmd = [TOOL, "-i", str(d / in1), "-I", str(d / in2), "-o", str(o1), "-O", str(o2)] + (["-j", str(js)] if json_out else []) + list(extra)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p, " ".join(["readqc"] + cmd[1:]), [f.read_bytes() if f.exists() else None for f in (o1, o2, js)]


def test_full_report_equals_the_restatement(files):
    d, t1, t2, want = files
    version = capi.lib().palace_version().decode()
    for tag, extra, ins, prm in (("full", ["--full-report"], ("r_1.fq", "r_2.fq"), rc.DEFAULTS), ("fullgz", ["--full-report"], ("r_1.fq.gz", "r_2.fq.gz"), rc.DEFAULTS),
                                 ("fullopt", ["--full-report", "-q", "20", "-l", "60", "-n", "2"], ("r_1.fq", "r_2.fq"),
                                  rc.params(qualified_quality=20, min_length=60, n_limit=2))):
        p, command, (o1, o2, js) = tool(d, tag, extra, *ins)
        assert p.returncode == 0 and p.stdout == b"" and p.stderr == b"", (tag, p.stderr)
        rep = rr.full_report(t1, t2, prm, version, command)
        got = json.loads(js)
        assert list(got) == list(rep), tag
        for key in rep:                                                      # (key by key: a failure names its part)
            assert got[key] == rep[key], (tag, key)
        res = rc.readqc(t1, t2, prm)
        assert o1 == res["out1"] and o2 == res["out2"], tag
    rep = rr.full_report(t1, t2, rc.DEFAULTS, version, "")
    assert rep["summary"]["sequencing"] == "paired end (140 cycles + 151 cycles)"
    before, after = rep["summary"]["before_filtering"], rep["summary"]["after_filtering"]
    assert 0 < after["q30_bases"] < after["q20_bases"] < before["q20_bases"] < before["total_bases"] and after["read2_mean_length"] < 151
    assert rep["insert_size"]["unknown"] > 100 and 30 < rep["insert_size"]["peak"] < 300 and rep["read2_after_filtering"]["total_cycles"] == 151
    assert max(rep["read1_before_filtering"]["content_curves"]["N"]) > 0


def test_outputs_and_plain_json_are_untouched(files):
    d, _, _, want = files
    p, _, (o1, o2, js) = tool(d, "plain")
    assert p.returncode == 0 and o1 == want["out1"] and o2 == want["out2"] and json.loads(js) == rc.report(want)
    p, _, (f1, f2, _) = tool(d, "withfull", ["--full-report"])
    assert p.returncode == 0 and f1 == o1 and f2 == o2


def test_full_report_needs_the_json_file(files):
    d, _, _, _ = files
    p, _, outs = tool(d, "nojson", ["--full-report"], json_out=False)
    assert p.returncode == 2 and p.stdout == b"" and outs == [None] * 3, p.stderr
    assert b"--full-report needs -j" in p.stderr
    assert [f.name for f in d.iterdir() if f.name.startswith("nojson")] == []
