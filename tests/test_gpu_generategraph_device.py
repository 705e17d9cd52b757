"""`generateGraph --bam-gpu` (the BAM inflated, CRC-checked, walked and decoded into the classify kernel's columns and SA items on the
device: palace_amd/host/bam_stream_device.hpp, palace_bam_columns / palace_bam_sa_items) against the host loader of the same binary:
every test runs the same command with and without the option and compares the bytes of what they write.  The kernels themselves:
tests/test_gpu_bam_columns.py."""
import os
import struct
import subprocess
import tempfile

import pytest
from hypothesis import HealthCheck, given, settings

from palace_amd import synth
from tests import graph_cases as gc
from tests.test_gpu_graph_fuzz import cases
from tests.test_host_bam_spec import EOF_MEMBER, bgzf_member, header

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENERATE_GRAPH = os.path.join(ROOT, "palace_amd", "bin", "generateGraph")
OPTS = ("PALACE_OPT_BAM_BATCH", "PALACE_OPT_BAM_CHUNK", "PALACE_TRACE")


def run(args, **opts):
    env = {k: v for k, v in os.environ.items() if k not in OPTS}
    env.update({k: str(v) for k, v in opts.items()})
    return subprocess.run([GENERATE_GRAPH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def own_lines(stderr):
    """stderr without the line the GPU machines' libdrm writes when its ids file is missing"""
    return [l for l in stderr.decode().splitlines() if not l.startswith("/opt/amdgpu/")]


def same_graph(d, args, bam, fai, depth="1", **opts):
    """the command on the host loader and with --bam-gpu: both succeed and write the same bytes, which are returned"""
    out_h, out_g = os.path.join(d, "host_graph.txt"), os.path.join(d, "gpu_graph.txt")
    h = run(list(args) + [bam, fai, out_h, depth])
    g = run(["--bam-gpu"] + list(args) + [bam, fai, out_g, depth], **opts)
    assert h.returncode == 0, h.stderr
    assert g.returncode == 0, g.stderr
    assert g.stdout == h.stdout
    text = open(out_h, "rb").read()
    assert open(out_g, "rb").read() == text
    return text, h, g


def test_adversarial_records_equal_the_host_mode():
    """30 derandomised examples of the strategy of tests/test_gpu_graph_fuzz.py, records straddling BGZF members of 700 bytes; the first
    example with ten records or more runs a second time with two members per batch and walk chunks of 256 bytes"""
    seen = {"examples": 0, "small_batches": 0, "junctions": 0}

    @settings(max_examples=30, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True, database=None)
    @given(cases())
    def check(case):
        targets, fai_text, recs, extra = case
        with tempfile.TemporaryDirectory(prefix="palace_bamgpu_") as d:
            bam, fai = os.path.join(d, "t.bam"), os.path.join(d, "g.fastg.fai")
            synth.write_bam(bam, targets, recs, block=700)
            open(fai, "w").write(fai_text)
            text, _, _ = same_graph(d, ["--min-count", "1", *extra], bam, fai)
            seen["examples"] += 1
            seen["junctions"] += text.count(b"JUNC")
            if len(recs) >= 10 and not seen["small_batches"]:
                assert same_graph(d, ["--min-count", "1", *extra], bam, fai, PALACE_OPT_BAM_BATCH=2, PALACE_OPT_BAM_CHUNK=256)[0] == text
                seen["small_batches"] = 1

    check()
    assert seen["examples"] >= 30 and seen["small_batches"] == 1 and seen["junctions"] > 0


def test_auto_depth(tmp_path):
    """<avgDepth> = auto on the depth hand case: the segments come from palace_bam_match_segments, the logged line is the same"""
    bam, fai = str(tmp_path / "d.bam"), str(tmp_path / "g.fastg.fai")
    synth.write_bam(bam, gc.DEPTH_TARGETS, gc.depth_records())
    open(fai, "w").write("%s;\t1\t0\t60\t61\n" % gc.DEPTH_TARGETS[0][0])
    text, h, g = same_graph(str(tmp_path), ["--min-count", "1"], bam, fai, depth="auto")
    depth_line = "Average sequencing depth: " + gc.DEPTH_TEXT
    assert depth_line in own_lines(h.stderr) and own_lines(g.stderr) == own_lines(h.stderr)
    assert text.count(b"SEG") == len(gc.DEPTH_TARGETS)
    g = run(["--bam-gpu", bam, fai, str(tmp_path / "traced.txt"), "auto"], PALACE_TRACE=1)
    line = [l for l in g.stderr.decode().split("\n") if l.startswith("[generateGraph] bam-gpu ms:")]
    assert g.returncode == 0 and len(line) == 1
    for lap in ("index", "header", "upload", "inflate", "crc", "walk", "columns", "sa", "records", "SA items"):
        assert lap in line[0]


def test_fused_stage04_outputs(tmp_path):
    """the one-process stage-04 call on the smallest sample of tests/test_gpu_stage04.py: every output file byte for byte"""
    rng = synth.rng_for(15)
    targets, fai_text, recs, avg = synth.random_graph_case(rng, 80, 6000)
    names, lens = [t[0] for t in targets], [t[1] for t in targets]
    P = lambda n: str(tmp_path / n)
    synth.write_bam(P("t.bam"), targets, recs, block=30000)
    for k, v in dict(fastg_fai=fai_text, **synth.filter_side_files(rng, names, lens)).items():
        open(P(k), "w").write(v)
    outs = ("graph", "pre", "filt", "hits", "lin", "cyc", "nodup", "all")

    def call(tag, *mode):
        p = run([*mode, "--min-count", "2", "--hit-seqs", P("hit_seqs"), "--node-scores", P("node_scores"), "--blast", P("blast"), "--fasta-fai", P("fasta_fai"),
                 "--paths", P("contigs_paths"), "--filtered-pre", P(f"{tag}_pre.txt"), "--filtered", P(f"{tag}_filt.txt"), "--all-hit-segs", P(f"{tag}_hits.txt"),
                 "--linear", P(f"{tag}_lin.txt"), "--cycle", P(f"{tag}_cyc.txt"), "--cycle-nodup", P(f"{tag}_nodup.txt"), "--all-result", P(f"{tag}_all.txt"),
                 "-i", "10", "-s", P("t.bam"), P("fastg_fai"), P(f"{tag}_graph.txt"), f"{avg:.6g}"])
        assert p.returncode == 0, p.stderr

    call("h")
    call("g", "--bam-gpu")
    for name in outs:
        assert open(P(f"g_{name}.txt"), "rb").read() == open(P(f"h_{name}.txt"), "rb").read(), name
    assert open(P("h_all.txt")).read().count("\t") > 5 and open(P("h_pre.txt")).read().count("JUNC") > 5


def graph_case():
    rng = synth.rng_for(4)
    targets, fai_text, recs, _ = synth.random_graph_case(rng, 60, 4000)
    return targets, fai_text, recs


def write_members(path, stream, size):
    with open(path, "wb") as f:
        for a in range(0, len(stream), size):
            f.write(bgzf_member(stream[a:a + size]))
        f.write(EOF_MEMBER)


def rejected_like_the_host(tmp_path, bam, fai):
    """exit 1, nothing on stdout, the host mode's stderr line, no output file"""
    out_h, out_g = str(tmp_path / "bad_h.txt"), str(tmp_path / "bad_g.txt")
    h, g = run([bam, fai, out_h, "1"]), run(["--bam-gpu", bam, fai, out_g, "1"])
    assert g.returncode == h.returncode == 1 and g.stdout == b"" == h.stdout
    assert len(own_lines(g.stderr)) == 1 and own_lines(g.stderr) == own_lines(h.stderr)
    assert not os.path.exists(out_g)


def test_damaged_files(tmp_path):
    targets, fai_text, recs = graph_case()
    bam, fai = str(tmp_path / "x.bam"), str(tmp_path / "g.fastg.fai")
    open(fai, "w").write(fai_text)
    synth.write_bam(bam, targets, recs, block=4096, level=0)
    good = open(bam, "rb").read()
    open(bam, "wb").write(good[:len(good) - 28 - 40])                         # truncated inside the last data member
    rejected_like_the_host(tmp_path, bam, fai)
    open(bam, "wb").write(b"\x00" + good[1:])                                 # the gzip magic
    rejected_like_the_host(tmp_path, bam, fai)
    open(bam, "wb").write(bgzf_member(b"not a BAM at all, " * 20) + EOF_MEMBER)     # the BAM magic
    rejected_like_the_host(tmp_path, bam, fai)
    # one byte of a stored member's data flipped: only the CRC-32 of the trailer tells, and only this mode compares it
    second = struct.unpack_from("<H", good, 16)[0] + 1
    assert good[second + 18] & 7 == 1
    at = second + 18 + 5 + 1000
    open(bam, "wb").write(good[:at] + bytes([good[at] ^ 0x01]) + good[at + 1:])
    out = str(tmp_path / "crc.txt")
    g = run(["--bam-gpu", bam, fai, out, "1"])
    assert g.returncode == 1 and g.stdout == b"" and len(own_lines(g.stderr)) == 1 and "CRC-32 mismatch" in own_lines(g.stderr)[0]
    assert not os.path.exists(out)


def test_malformed_record_mid_file(tmp_path):
    """l_read_name 0 in a record at three fifths of the file: the stream ends there for both loaders, the records in front are used"""
    targets, fai_text, recs = graph_case()
    enc = [r.encode() for r in recs]
    k = len(enc) * 3 // 5
    bad = bytearray(enc[k])
    bad[4 + 8] = 0
    bam, fai = str(tmp_path / "m.bam"), str(tmp_path / "g.fastg.fai")
    open(fai, "w").write(fai_text)
    args = ["--min-count", "1"]
    write_members(bam, header(targets) + b"".join(enc[:k]) + bytes(bad) + b"".join(enc[k + 1:]), 3000)
    cut = same_graph(str(tmp_path), args, bam, fai)[0]
    write_members(bam, header(targets) + b"".join(enc[:k]), 3000)
    assert same_graph(str(tmp_path), args, bam, fai)[0] == cut                 # ... and is the graph of the records in front of it
    write_members(bam, header(targets) + b"".join(enc), 3000)
    assert same_graph(str(tmp_path), args, bam, fai)[0] != cut
