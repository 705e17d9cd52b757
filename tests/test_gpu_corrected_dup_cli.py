"""bin/corrected_dup and scripts/corrected_dup.py end to end: every case of tests/golden/corrected_dup_cases.npz -- what the
reference's script wrote -- with the depth handed over as `--contig-depth`, byte for byte, with an empty cycle_nodup file and the
script's warning lines as the only stdout; six of them again through a BAM that palace_amd.synth.write_bam writes to the same
per-contig sums, read by the device loader, with identical results; and every rejection of DESIGN.md 8 with its message, exit
code 1 and no final.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

from palace_amd import synth
from tests import corrected_dup_cases as cd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(ROOT, "palace_amd", "bin", "corrected_dup")
SCRIPT = os.path.join(ROOT, "palace_amd", "scripts", "corrected_dup.py")
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "corrected_dup_cases.npz"))
NAMES = sorted({k.split("__")[0] for k in GOLDEN.files})
THROUGH_BAM = ["border", "two_units", "both_strands", "unknown_and_bare", "tandem_by_depth", "doubled_gone"]


def golden_case(name):
    case = {k: GOLDEN[f"{name}__{k}"].tobytes() for k in ("fai", "cycle", "final", "before_cut", "depth")}
    case["min_len"] = int(GOLDEN[name + "__min_len"][0])
    return case


def run_tool(d, case, depth="table", tool=(BINARY,)):
    d = str(d)
    for fn, key in (("edges.fasta.fai", "fai"), ("cycle.txt", "cycle"), ("final_all.txt", "final"), ("before_cut.txt", "before_cut"), ("depth.tsv", "depth")):
        open(os.path.join(d, fn), "wb").write(case[key])
    head = ["--contig-depth", os.path.join(d, "depth.tsv")] if depth == "table" else []
    bam = os.path.join(d, "reads.bam") if depth == "bam" else os.path.join(d, "absent.bam")
    p = subprocess.run(list(tool) + head + [os.path.join(d, "out"), "prefix", os.path.join(d, "cycle.txt"), os.path.join(d, "final_all.txt"), "final.txt", "final.fasta",
                                            os.path.join(d, "edges.fasta"), "cycle_nodup.txt", bam, os.path.join(d, "before_cut.txt"), str(case["min_len"])],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return p, os.path.join(d, "out", "final.txt"), os.path.join(d, "out", "cycle_nodup.txt")


def test_the_golden_file_is_the_catalogue():
    cases = cd.golden_inputs()
    assert len(NAMES) >= 60 and set(NAMES) <= set(cases)
    for name in NAMES:
        assert golden_case(name) == cases[name], name


@pytest.mark.parametrize("name", NAMES)
def test_golden_case_with_contig_depth(tmp_path, name):
    p, out, nodup = run_tool(tmp_path, golden_case(name))
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == GOLDEN[name + "__out"].tobytes()
    assert os.path.getsize(nodup) == 0
    assert p.stdout == GOLDEN[name + "__stdout"].tobytes()
    assert not os.path.exists(out + ".tmp")


def write_depth_bam(path, case):
    """reads whose per-contig depth sums and covered positions are the table's: sum // covered reads over the covered positions and
    one more over the first sum % covered of them"""
    fai, depth = cd.parse_inputs(case)
    targets = [(n, fai[n]) for n in fai if n in depth]
    records = []
    for tid, (name, length) in enumerate(targets):
        total, covered = depth[name]
        if not covered:
            continue
        assert total >= covered and covered <= length
        records += [synth.BamRecord(f"r{tid}_{k}", 0, tid, 0, 60, f"{covered}M") for k in range(total // covered)]
        if total % covered:
            records.append(synth.BamRecord(f"r{tid}_x", 0, tid, 0, 60, f"{total % covered}M"))
    synth.write_bam(path, targets, records)


@pytest.mark.parametrize("name", THROUGH_BAM)
def test_golden_case_through_a_bam(tmp_path, name):
    case = golden_case(name)
    write_depth_bam(str(tmp_path / "reads.bam"), case)
    p, out, nodup = run_tool(tmp_path, case, depth="bam")
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == GOLDEN[name + "__out"].tobytes() and os.path.getsize(nodup) == 0 and p.stdout == b""


def test_the_script_starts_the_executable(tmp_path):
    p, out, _ = run_tool(tmp_path, golden_case("before_cut"), tool=(sys.executable, SCRIPT))
    assert p.returncode == 0, p.stderr
    assert open(out, "rb").read() == GOLDEN["before_cut__out"].tobytes() and p.stdout == b""


A, B = cd.edge(1, 900, "10.0"), cd.edge(2, 100, "10.5")
CONTIGS = [(A, 900), (B, 100), ("CTG001", 70)]
REJECTIONS = [
    ("cycle", dict(cycles=[[A + "+"], ["EDGE_9_length_5_cov_1.0+"]]), 2, "'EDGE_9_length_5_cov_1.0' is no sequence of the index"),
    ("cycle", dict(cycles=[[A + "+"], [], [B + "+"]]), 2, "a blank line"),
    ("before_cut", dict(raw_before=b"%s+\t%s+\n" % (A.encode(), B.encode())), 1, "not exactly one ':'"),
    ("before_cut", dict(raw_before=b"%s+:%s+\n%s+:%s+:%s+\n" % ((A.encode(), B.encode()) + (A.encode(),) * 3)), 2, "not exactly one ':'"),
    ("before_cut", dict(raw_before=b"\n"), 1, "not exactly one ':'"),
    ("final", dict(finals=[[A + "+"], [B]]), 2, f"'{B}' does not end in '+' or '-'"),
    ("final", dict(finals=[[A + "+" + B + "-"]]), 1, f"'{A}+{B}-' holds a '+', '-' or ':' inside"),
    ("final", dict(finals=[[A + "+"], [A + "+"], ["x" + A + "+"]]), 3, f"'x{A}+' matches the EDGE pattern in part only"),
    ("final", dict(finals=[[A + "+"], ["NOPE+"], [B]]), 2, "'NOPE' is no sequence of the index"),                      # the smallest faulty line, whatever its kind
    ("before_cut", dict(before=[([A + "+"], ["NOPE-"])]), 1, "'NOPE' is no sequence of the index"),
]


@pytest.mark.parametrize("k", range(len(REJECTIONS)))
def test_rejections(tmp_path, k):
    which, change, line, reason = REJECTIONS[k]
    case = cd.make_case(CONTIGS, change.get("cycles", [[A + "+", B + "+"]]), change.get("finals", [[B + "-"]]), change.get("before", ()),
                        {n: (10 * ln, ln) for n, ln in CONTIGS})
    if "raw_before" in change:
        case["before_cut"] = change["raw_before"]
    p, out, _ = run_tool(tmp_path, case)
    file = {"cycle": "cycle.txt", "final": "final_all.txt", "before_cut": "before_cut.txt"}[which]
    assert p.returncode == 1 and p.stdout == b""
    assert f"{os.path.join(str(tmp_path), file)}: line {line}: {reason}" in p.stderr.decode(), p.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp")
    with pytest.raises(cd.Rejected):
        cd.corrected_dup(case)
