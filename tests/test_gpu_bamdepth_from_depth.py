"""`bamdepth --from-depth` (palace_amd/host/depth_read.hpp): the depth file the other modes write, read back on the device -- the same
number and the same per-contig table as from the BAM --, foreign BGZF against the Python restatement, and what is rejected."""
import gzip
import os
import struct
import subprocess
import zlib

import pytest

from palace_amd import synth
from tests import depth_cases as dc
from tests import tabix_reader as tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMDEPTH = os.path.join(ROOT, "palace_amd", "bin", "bamdepth")
KNOBS = ("PALACE_OPT_DEPTHIN_BATCH", "PALACE_OPT_DEPTHIN_WINDOW", "PALACE_TRACE")


def bamdepth(args, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update({k: str(v) for k, v in knobs.items()})
    return subprocess.run([BAMDEPTH] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def rejected(p, path):
    return p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"bamdepth: ") and p.stderr.count(b"\n") == 1 and str(path).encode() in p.stderr


def member(data: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(data) + c.flush()
    return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(body) + 25) + body + struct.pack("<II", zlib.crc32(data), len(data))


def foreign_bgzf(text: bytes, rng, level: int, eof: bool, empties: bool = True) -> bytes:
    out, p, k = [], 0, 0
    while p < len(text):
        n = int(rng.integers(1, 65281)) if k % 3 else int(rng.integers(1, 300))
        out.append(member(text[p:p + n], level))
        p += n
        k += 1
        if empties and k % 4 == 0:
            out.append(member(b"", level))
    return b"".join(out) + (tr.EOF_MEMBER if eof else b"")


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("from_depth")
    rng = synth.rng_for(3)
    # 200 contigs, ~100 of them covered, 0.5 MB of depth text in 10 members: with PALACE_OPT_DEPTHIN_WINDOW=64 the text is ~9 000 windows,
    # each a round trip to the device, so the text is kept this small
    targets, _, recs, _ = synth.random_graph_case(rng, 200, 100, long_mode=False)
    bam = str(d / "t.bam")
    synth.write_bam(bam, targets, sorted(recs, key=lambda r: (r.tid if r.tid >= 0 else 1 << 30, r.pos)))
    mean, table = bamdepth([bam]), bamdepth(["--per-contig", bam])
    assert mean.returncode == 0 and table.returncode == 0 and table.stdout.count(b"\n") > 50
    files = {}
    for mode in ("--depth-gz", "--depth-gz-gpu"):
        gz = str(d / (mode.strip("-") + ".depth.gz"))
        p = bamdepth([mode, gz, bam])
        assert p.returncode == 0 and p.stdout == mean.stdout, p.stderr
        files[mode] = gz
    text = tr.TabixFile(files["--depth-gz"]).text
    plain = str(d / "t.depth")
    open(plain, "wb").write(text)
    files["plain"] = plain
    return {"dir": d, "mean": mean.stdout, "table": table.stdout, "files": files, "text": text}


def test_round_trips(case):
    assert len(tr.bgzf_members(open(case["files"]["--depth-gz"], "rb").read())) > 3
    for kind, path in case["files"].items():
        settings = [{}] + ([{"PALACE_OPT_DEPTHIN_WINDOW": w} for w in (64, 4099)] if kind == "plain" else [{"PALACE_OPT_DEPTHIN_BATCH": b} for b in (1, 2, 3)])
        for knobs in settings:
            p, q = bamdepth(["--from-depth", path], **knobs), bamdepth(["--from-depth", "--per-contig", path], **knobs)
            assert p.returncode == 0 and q.returncode == 0, (kind, knobs, p.stderr, q.stderr)
            assert p.stdout == case["mean"] and q.stdout == case["table"], (kind, knobs)
    p = bamdepth(["--from-depth", case["files"]["--depth-gz"]], PALACE_TRACE=1)
    assert p.returncode == 0 and p.stdout == case["mean"] and b"[bamdepth] from-depth ms: index" in p.stderr and b"members inflated on the host" in p.stderr


def foreign_text(rng, integral):
    names = [b"zeta", b"alpha contig", b"m" * 200, b"b"]
    lines = []
    for rep in range(3):                                 # unsorted, and every contig comes back twice
        for name in names:
            for p in range(1, int(rng.integers(500, 4000))):
                lines.append(b"%s\t%d\t%d" % (name, p + 10000 * rep, 0 if p % 7 == 0 else int(rng.integers(0, 3000))))
    if integral:                                         # one more line makes the sum a multiple of the line count
        _, n, total, _, _ = dc.restate(b"\n".join(lines) + b"\n")
        lines.append(b"b\t99999\t%d" % ((n + 1) - total % (n + 1)))
    return b"\n".join(lines) + b"\n"


@pytest.mark.parametrize("level,eof,integral", [(1, True, False), (9, False, True)])
def test_foreign_bgzf(tmp_path, level, eof, integral):
    rng = synth.rng_for(20 + level)
    text = foreign_text(rng, integral)
    _, n, total, per, _ = dc.restate(text)
    assert (total % n == 0) == integral and b"\t0\n" in text
    path = tmp_path / "foreign.depth.gz"
    path.write_bytes(foreign_bgzf(text, rng, level, eof))
    want_table = b"".join(b"%s\t%d\t%d\n" % (k, v[0], v[1]) for k, v in per.items())
    for knobs in ({}, {"PALACE_OPT_DEPTHIN_BATCH": 2}, {"PALACE_OPT_DEPTHIN_BATCH": 5}):
        p, q = bamdepth(["--from-depth", path], **knobs), bamdepth(["--from-depth", "--per-contig", path], **knobs)
        assert p.returncode == 0 and q.returncode == 0, (p.stderr, q.stderr)
        assert p.stdout == dc.awk_number(total, n) + b"\n" and q.stdout == want_table
    # the same text without its final LF, plain
    plain = tmp_path / "foreign.depth"
    plain.write_bytes(text[:-1])
    p, q = bamdepth(["--from-depth", plain], PALACE_OPT_DEPTHIN_WINDOW=70000), bamdepth(["--from-depth", "--per-contig", plain])
    assert p.stdout == dc.awk_number(total, n) + b"\n" and q.stdout == want_table


def test_empty_inputs(tmp_path):
    a, b = tmp_path / "eof.depth.gz", tmp_path / "empty.depth"
    a.write_bytes(tr.EOF_MEMBER)
    b.write_bytes(b"")
    for path in (a, b):
        p, q = bamdepth(["--from-depth", path]), bamdepth(["--from-depth", "--per-contig", path])
        assert p.returncode == 2 and p.stdout == b"" and b"division by zero" in p.stderr
        assert q.returncode == 0 and q.stdout == b"" and q.stderr == b""


def test_rejections(tmp_path):
    rng = synth.rng_for(31)
    lines = [b"c%d\t%d\t%d" % (p // 3000, p, p % 50) for p in range(1, 12001)]
    text = b"\n".join(lines) + b"\n"
    good = foreign_bgzf(text, rng, 6, True, empties=False)
    mem = tr.bgzf_members(good)
    path = tmp_path / "r.depth.gz"
    path.write_bytes(good)
    assert bamdepth(["--from-depth", path]).returncode == 0
    second = mem[1][0]                                   # offset of the second member
    for at in (second + 18 + 5, second - 8 + 1):         # inside the second member's data, inside the first member's CRC
        blob = bytearray(good)
        blob[at] ^= 0x20
        path.write_bytes(bytes(blob))
        for args in (["--from-depth", path], ["--from-depth", "--per-contig", path]):
            p = bamdepth(args)
            assert rejected(p, path) and b"offset" in p.stderr, p.stderr
    path.write_bytes(good[:second + 40])                 # truncated inside a member
    p = bamdepth(["--from-depth", path])
    assert rejected(p, path) and b"offset %d" % second in p.stderr, p.stderr
    path.write_bytes(good + b"trailing bytes, more than a header's worth")
    assert rejected(bamdepth(["--from-depth", path]), path)
    path.write_bytes(gzip.compress(text))                # gzip, not BGZF
    p = bamdepth(["--from-depth", path])
    assert rejected(p, path) and b"not BGZF" in p.stderr, p.stderr
    # a bad line at a known number, in the second batch
    bad_at = 9000
    broken = list(lines)
    broken[bad_at - 1] = b"c3\t9000\t-1"
    blob = foreign_bgzf(b"\n".join(broken) + b"\n", synth.rng_for(32), 6, True, empties=False)
    members = tr.bgzf_members(blob)
    first_two = sum(len(m[1]) for m in members[:2])
    assert len(members) >= 3 and b"\n".join(broken[:bad_at]).__len__() > first_two      # the line lies behind the first batch of two members
    path.write_bytes(blob)
    for args in (["--from-depth", path], ["--from-depth", "--per-contig", path]):
        p = bamdepth(args, PALACE_OPT_DEPTHIN_BATCH=2)
        assert rejected(p, path) and b": line 9000: " in p.stderr, p.stderr
    plain = tmp_path / "r.depth"
    plain.write_bytes(b"\n".join(broken) + b"\n")
    p = bamdepth(["--from-depth", plain], PALACE_OPT_DEPTHIN_WINDOW=4099)
    assert rejected(p, plain) and b": line 9000: " in p.stderr
