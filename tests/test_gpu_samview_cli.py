"""The `samview` executable and `bamsort --sam` end to end on SAM texts built here: the file is read back member by member with zlib
(BSIZE, CRC-32 and ISIZE checked by the reader) and its stream must be the header plus the records of the Python restatement
(tests/sam_cases.py), never the device's.  Two second opinions do not go through the restatement: `bamdepth` on the output against
a brute-force count over the SAM lines, and `bamsort --sam` against `bamsort` on samview's output, byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import sam_cases as sc
from tests.tabix_reader import EOF_MEMBER, bgzf_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
SAMVIEW, BAMSORT, BAMDEPTH = (os.path.join(BIN, n) for n in ("samview", "bamsort", "bamdepth"))
MEMBER = 0xff00


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host")] + [os.path.join("..", "bin", n) for n in ("samview", "bamsort", "bamdepth")],
                   check=True, stdout=subprocess.DEVNULL)


def run(tool, args, stdin=b""):
    return subprocess.run([tool] + [str(a) for a in args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def ok(tool, args, stdin=b""):
    p = run(tool, args, stdin)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode()
    return p.stdout


def stream_of(data, stored):
    """the file's members (each checked by the reader) -> the inflated stream; the cut into members is bgzip's"""
    mem = bgzf_members(data)
    assert data[-28:] == EOF_MEMBER and mem[-1][1] == b""
    sizes = [len(x) for _, x in mem[:-1]]
    assert all(s == MEMBER for s in sizes[:-1]) and 0 < sizes[-1] <= MEMBER
    if stored:                                       # one final stored block per member: 18 + 5 + the bytes + 8
        for (at, x), nxt in zip(mem[:-1], mem[1:]):
            assert nxt[0] - at == 31 + len(x) and data[at + 18] == 1 and data[at + 19:at + 21] == len(x).to_bytes(2, "little")
            assert data[at + 23:at + 23 + len(x)] == x
    return b"".join(x for _, x in mem)


def main_text():
    rng = np.random.default_rng(21)
    lines = []
    for _ in range(3000):
        f = sc.valid_line(rng).split(b"\t")
        f[3] = b"%d" % int(rng.integers(0, 800))                             # (a place a .bai can hold)
        lines.append(b"\t".join(f))
    return sc.HEADER + b"\n".join(lines) + b"\n"


@pytest.fixture(scope="module")
def main_case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("samview_main")
    text = main_text()
    recs, _, first = sc.text_verdict(text, 0x800)
    assert first is None and 1500 < len(recs) < 3000
    want = sc.bam_header(text) + b"".join(recs)
    assert len(want) > 3 * MEMBER
    (tmp / "in.sam").write_bytes(text)
    return dict(tmp=tmp, text=text, want=want, sam=tmp / "in.sam")


def test_the_drivers_command_line_from_stdin_and_dash_o_from_a_file(main_case):
    piped = ok(SAMVIEW, ["-@", 4, "-F", "0x0800", "-buS", "-"], main_case["text"])
    assert stream_of(piped, True) == main_case["want"]
    out = main_case["tmp"] / "u.bam"
    assert ok(SAMVIEW, ["-F", 2048, "-b", "-u", "-o", out, main_case["sam"]]) == b""
    assert out.read_bytes() == piped


def test_without_u_the_members_are_the_device_coders(main_case):
    out = main_case["tmp"] / "z.bam"
    assert ok(SAMVIEW, ["-F0x800", "-bho", out, main_case["sam"]]) == b""
    data = out.read_bytes()
    assert stream_of(data, False) == main_case["want"]
    assert len(data) < len(main_case["want"])
    assert stream_of(ok(SAMVIEW, ["-b", main_case["sam"]]), False) == sc.bam_header(main_case["text"]) + b"".join(sc.text_verdict(main_case["text"])[0])


def test_bamsort_sam_is_bamsort_on_samviews_output(main_case):
    tmp = main_case["tmp"]
    ok(SAMVIEW, ["-F", "0x0800", "-bu", "-o", tmp / "tmp.bam", main_case["sam"]])
    assert ok(BAMSORT, ["-@", 4, tmp / "tmp.bam", "-O", "BAM", "-o", tmp / "two.bam", "--bai"]) == b""
    assert ok(BAMSORT, ["--sam", "-F", "0x0800", "-@", 4, main_case["sam"], "-O", "BAM", "-o", tmp / "one.bam", "--bai"]) == b""
    assert ok(BAMSORT, ["--sam", "-F2048", "-", "-o", tmp / "pipe.bam", "--bai"], main_case["text"]) == b""
    for name in ("one.bam", "pipe.bam"):
        assert (tmp / name).read_bytes() == (tmp / "two.bam").read_bytes() and (tmp / (name + ".bai")).read_bytes() == (tmp / "two.bam.bai").read_bytes()
    assert len((tmp / "two.bam.bai").read_bytes()) > 100
    # ... and the sorted stream holds the restatement's records, each once
    got = stream_of((tmp / "one.bam").read_bytes(), False)
    recs = sc.text_verdict(main_case["text"], 0x800)[0]
    at, seen = len(got) - sum(len(r) for r in recs), []                     # (the header grew by its SO:coordinate, the records did not)
    while at < len(got):
        n = 4 + int.from_bytes(got[at:at + 4], "little")
        seen.append(got[at:at + n])
        at += n
    assert sorted(seen) == sorted(recs)


def test_bamdepth_on_the_output_counts_what_the_lines_say(tmp_path):
    """the second opinion: M, = and X bases of every line whose flag has none of 0x4, 0x100, 0x200, 0x400 (and 0x800: dropped), counted here"""
    rng = np.random.default_rng(23)
    targets = [(b"c0", 5000), (b"c1", 900)]
    header = b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % t for t in targets)
    depth = {n: np.zeros(l, np.int64) for n, l in targets}
    lines = []
    for name, length in targets:
        for pos in sorted(int(x) for x in rng.integers(1, length - 300, size=400)):
            ops = [(int(rng.integers(1, 40)), b"MIDNS=X"[int(rng.integers(0, 7))]) for _ in range(int(rng.integers(1, 6)))]
            flag = int(rng.choice([0, 16, 99, 147, 256, 512, 1024, 2048, 4, 2064]))
            qlen = sum(n for n, o in ops if o in b"MIS=X")
            lines.append(b"r\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*" % (flag, name, pos, b"".join(b"%d%c" % x for x in ops), b"A" * qlen if qlen else b"*"))
            at = pos - 1
            for n, o in ops:
                if o in b"M=X" and not flag & (4 | 256 | 512 | 1024 | 2048):
                    depth[name][at:at + n] += 1
                if o in b"MDN=X":
                    at += n
    lines.append(b"u\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*")
    sam, bam = tmp_path / "in.sam", tmp_path / "out.bam"
    sam.write_bytes(header + b"\n".join(lines) + b"\n")
    ok(SAMVIEW, ["-F", "0x0800", "-buS", "-o", bam, sam])
    total, covered = sum(int(d.sum()) for d in depth.values()), sum(int((d > 0).sum()) for d in depth.values())
    assert covered > 1000
    assert ok(BAMDEPTH, [bam]).decode().strip() == "%.6g" % (total / covered)
    want = b"".join(b"%s\t%d\t%d\n" % (n, int(depth[n].sum()), int((depth[n] > 0).sum())) for n, _ in targets)
    assert ok(BAMDEPTH, ["--per-contig", bam]) == want


def test_a_text_without_alignment_lines(tmp_path):
    for text in (sc.HEADER, b""):
        assert stream_of(ok(SAMVIEW, ["-bu", "-"], text), True) == sc.bam_header(text)


def test_a_grammar_error_leaves_no_file_and_an_empty_stdout(tmp_path):
    lines = sc.generated(7, 60, damaged=0.0)
    lines = [l for l in lines if l and not l.startswith(b"@")]
    bad = lines[:40] + [sc.HAND_ERRORS[7][0]] + lines[40:] + [b"", b"@CO\tlate"]
    sam, out = tmp_path / "in.sam", tmp_path / "out.bam"
    for text, line in ((sc.HEADER + b"\n".join(bad) + b"\n", 5 + 41), (sc.HEADER + b"\n".join(lines) + b"\n\n@CO\n", 5 + len(lines) + 1),
                       (b"@SQ\tSN:a\tLN:5\n@SQ\tSN:a\tLN:5\n", 2), (sc.HEADER + sc.SPEC_READS[0] + b"\tXF:f:1.5\n", 6)):
        sam.write_bytes(text)
        for args, stdin in ((["-F", "0x0800", "-buS", "-"], text), (["-b", "-o", out, sam], b"")):
            p = run(SAMVIEW, args, stdin)
            assert p.returncode == 1 and p.stdout == b"" and p.stderr.count(b"\n") == 1
            assert re.match(rb"samview: line %d: \S" % line, p.stderr), p.stderr
        if line != 2:
            p = run(BAMSORT, ["--sam", "-o", out, "--bai", sam])
            assert p.returncode == 1 and p.stdout == b"" and re.match(rb"bamsort: \S*in.sam: line %d: \S" % line, p.stderr), p.stderr
        assert sorted(os.listdir(tmp_path)) == ["in.sam"]
    assert b"type f" in p.stderr                                             # the float tag's message names the type
