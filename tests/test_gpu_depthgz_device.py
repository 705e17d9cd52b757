"""`bamdepth --depth-gz-gpu` (palace_amd/host/depthgz_device.hpp: depth text, CRC-32, DEFLATE and the index's offsets on the device)
against the host mode `--depth-gz` and the checks of tests/test_host_depthgz.py: the same text, the same cut into members, the same
index once virtual offsets are mapped back to text offsets, the same number on stdout."""
import os
import subprocess

import pytest

from palace_amd import synth
from tests import tabix_reader as tr
from tests.test_host_depthgz import expected_depth_text

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMDEPTH = os.path.join(ROOT, "palace_amd", "bin", "bamdepth")


def run(tmp_path, targets, records, mode="--depth-gz-gpu", tag="g", batch=None):
    bam, gz = str(tmp_path / "t.bam"), str(tmp_path / f"{tag}.depth.gz")
    if not os.path.exists(bam):
        synth.write_bam(bam, targets, records)
    env = dict(os.environ)
    env.pop("PALACE_OPT_DEPTHGZ_BATCH", None)
    if batch:
        env["PALACE_OPT_DEPTHGZ_BATCH"] = str(batch)
    p = subprocess.run([BAMDEPTH, mode, gz, bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    return p, gz


def tbi_in_text_offsets(f):
    """the index with every virtual offset mapped to a text offset through the file's own member table"""
    refs = []
    for r in f.tbi["refs"]:
        bins = {b: ([(f._abs(a), f._abs(e)) for a, e in ch] if b != 37450 else [(f._abs(ch[0][0]), f._abs(ch[0][1])), ch[1]])
                for b, ch in r["bins"].items()}
        refs.append((bins, [f._abs(o) for o in r["ioff"]]))
    return f.tbi["names"], refs


def test_hand_derived_index(tmp_path):
    """the fixture of tests/test_host_depthgz.py::test_hand_derived_index: the numbers worked out by hand there"""
    targets = [("c1", 100), ("c2", 20000)]
    recs = [synth.BamRecord("r1", 0, 0, 10, 60, "5M"), synth.BamRecord("r2", 0, 1, 16380, 60, "10M")]
    p, gz = run(tmp_path, targets, recs)
    assert p.returncode == 0, p.stderr
    assert p.stdout == b"1\n"
    data = open(gz, "rb").read()
    mem = tr.bgzf_members(data)
    assert len(mem) == 2 and mem[0][0] == 0 and mem[1][1] == b"" and data[-28:] == tr.EOF_MEMBER
    want = b"".join(b"c1\t%d\t1\n" % q for q in range(11, 16)) + b"".join(b"c2\t%d\t1\n" % q for q in range(16381, 16391))
    assert mem[0][1] == want and len(want) == 150
    tbi = tr.read_tbi(gz + ".tbi")
    assert (tbi["format"], tbi["col_seq"], tbi["col_beg"], tbi["col_end"], tbi["meta"], tbi["skip"]) == (0, 1, 2, 2, ord("#"), 0)
    assert tbi["names"] == [b"c1", b"c2"] and tbi["n_no_coor"] == 0
    c1, c2 = tbi["refs"]
    assert c1["bins"] == {4681: [(0, 40)], 37450: [(0, 40), (5, 0)]} and c1["ioff"] == [0]
    assert c2["bins"] == {4681: [(40, 84)], 4682: [(84, 150)], 37450: [(40, 150), (10, 0)]} and c2["ioff"] == [40, 84]
    f = tr.TabixFile(gz)
    assert f.fetch("c2", 16383, 16385) == [b"c2\t16384\t1\n", b"c2\t16385\t1\n"]
    assert f.fetch("c1") == [b"c1\t%d\t1\n" % q for q in range(11, 16)]


@pytest.mark.parametrize("seed,long_mode", [(3, False), (4, True)])
def test_random_bam_equals_the_host_mode(tmp_path, seed, long_mode):
    rng = synth.rng_for(seed)
    targets, _, recs, _ = synth.random_graph_case(rng, 60 if long_mode else 300, 6000 if long_mode else 20000, long_mode=long_mode)
    extra = []
    for k in range(200):                      # the flags samtools skips, D / N / S / I / = / X, reads over the contig end
        t = int(rng.integers(0, len(targets)))
        L = targets[t][1]
        cig = ["20M5D30M", "10S40M", "25M3I25M2N20M", "30=5X15M", "50M"][k % 5]
        extra.append(synth.BamRecord(f"x{k}", [0, 0x400, 0x100, 0x200, 0x4, 0x800, 16][k % 7], t, int(rng.integers(0, max(1, L - 10))), 60, cig))
    recs = sorted(recs + extra, key=lambda r: (r.tid if r.tid >= 0 else 1 << 30, r.pos))
    p, gz = run(tmp_path, targets, recs)
    assert p.returncode == 0, p.stderr
    ph, gz_h = run(tmp_path, targets, recs, mode="--depth-gz", tag="h")
    assert ph.returncode == 0, ph.stderr
    lines, per_contig, total, nr = expected_depth_text(targets, recs)
    f, h = tr.TabixFile(gz), tr.TabixFile(gz_h)
    assert f.text == b"".join(lines)
    assert f.text == h.text and [len(x) for _, x in f.members] == [len(x) for _, x in h.members] and len(f.members) > 3
    assert tbi_in_text_offsets(f) == tbi_in_text_offsets(h)
    assert p.stdout == ph.stdout
    for name, mine in per_contig.items():
        assert f.fetch(name) == mine, name
    name = max(per_contig, key=lambda n: len(per_contig[n]))
    L = dict(targets)[name]
    for beg, end in [(0, 1), (16383, 16385), (16384, 40000), (L - 100, L), (L // 2, L // 2 + 20000)]:
        want = [l for l in per_contig[name] if beg < int(l.split(b"\t")[1]) <= end]
        assert f.fetch(name, beg, end) == want, (name, beg, end)
    # two members per batch: several batches, the same file
    p2, gz2 = run(tmp_path, targets, recs, tag="b2", batch=2)
    assert p2.returncode == 0 and p2.stdout == p.stdout
    assert open(gz2, "rb").read() == f.data and open(gz2 + ".tbi", "rb").read() == open(gz + ".tbi", "rb").read()


def test_text_ends_exactly_on_a_member_border(tmp_path):
    """4 080 lines of 16 bytes = 0xff00: one full member and the EOF member; the end of the contig's lines is the EOF member's
    offset with 0 inside it (BgzfTextWriter::voffset)"""
    targets = [("ctg_007", 20000)]
    p, gz = run(tmp_path, targets, [synth.BamRecord("r", 0, 0, 9999, 60, "4080M")])
    assert p.returncode == 0, p.stderr
    f = tr.TabixFile(gz)
    assert len(f.text) == 0xff00 == 4080 * 16 and f.text.startswith(b"ctg_007\t10000\t1\n") and f.text.endswith(b"ctg_007\t14079\t1\n")
    assert [len(x) for _, x in f.members] == [0xff00, 0]
    eof_at = f.members[1][0]
    assert f.tbi["refs"][0]["bins"][37450] == [(0, eof_at << 16), (4080, 0)]
    assert f.tbi["refs"][0]["bins"][4681] == [(0, eof_at << 16)]
    assert len(f.fetch("ctg_007")) == 4080


def test_contig_borders_in_the_global_coordinate(tmp_path):
    """contigs of length 0 and 1 between covered ones, a read that ends on its contig's last base followed by one at position 0 of
    the next contig, a read that runs past the end, a covered contig behind an uncovered one"""
    targets = [("a", 50), ("z0", 0), ("one", 1), ("b", 30), ("empty", 40), ("z1", 0), ("c", 25)]
    recs = [synth.BamRecord("r1", 0, 0, 40, 60, "10M"),        # a: 41 .. 50, ends on the last base
            synth.BamRecord("r2", 0, 2, 0, 60, "1M"),          # one: its single base
            synth.BamRecord("r3", 0, 3, 0, 60, "12M"),         # b: from position 0
            synth.BamRecord("r4", 0, 3, 20, 60, "30M"),        # b: runs past the end, cut at 30
            synth.BamRecord("r5", 0, 3, 25, 60, "5M"),
            synth.BamRecord("r6", 0, 6, 24, 60, "8M")]         # c: the very last position of all
    p, gz = run(tmp_path, targets, recs)
    assert p.returncode == 0, p.stderr
    ph, gz_h = run(tmp_path, targets, recs, mode="--depth-gz", tag="h")
    lines, per_contig, total, nr = expected_depth_text(targets, recs)
    f, h = tr.TabixFile(gz), tr.TabixFile(gz_h)
    assert f.text == b"".join(lines) == h.text
    assert b"b\t26\t2\n" in f.text and f.text.endswith(b"c\t25\t1\n")
    assert f.tbi["names"] == [b"a", b"one", b"b", b"c"]
    assert tbi_in_text_offsets(f) == tbi_in_text_offsets(h) and p.stdout == ph.stdout
    for name, mine in per_contig.items():
        assert f.fetch(name) == mine, name


def test_nothing_covered(tmp_path):
    p, gz = run(tmp_path, [("c1", 100)], [synth.BamRecord("r1", 4, -1, -1, 0, "")])
    assert p.returncode == 2 and b"division by zero" in p.stderr
    assert open(gz, "rb").read() == tr.EOF_MEMBER
    assert tr.read_tbi(gz + ".tbi")["names"] == []
