"""csrc/depth_line.hpp -- the grammar of a `samtools depth` line that the kernels of depth_parse.hip compile -- run on the host by
`hostdump depthline`, as built and under ASan + UBSan, against the Python restatement of tests/depth_cases.py line by line."""
import os
import subprocess

import pytest

from palace_amd import synth
from tests import depth_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
TOOLS = [os.path.join(ROOT, "palace_amd", "bin", t) for t in ("hostdump", "hostdump_asan")]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "hostdump"), os.path.join("..", "bin", "hostdump_asan")], check=True,
                   stdout=subprocess.DEVNULL)


def expected(lines):
    out = []
    for l in lines:
        p = dc.parse_line(l)
        out.append(b"bad" if p is None else b"ok %d %d %d" % (len(p[0]), p[1], p[2]))
    return out


def dump(tool, tmp_path, lines, final_lf=True):
    path = tmp_path / "lines.txt"
    path.write_bytes(b"\n".join(lines) + (b"\n" if final_lf else b""))
    p = subprocess.run([tool, "depthline", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]
    return p.stdout.split(b"\n")[:-1]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_case_table(tool, tmp_path):
    lines = dc.GOOD + dc.BAD + dc.GOOD
    got = dump(tool, tmp_path, lines)
    assert got == expected(lines)
    assert got[:len(dc.GOOD)] == [b"ok 1 1 1", b"ok 4000 5 7", b"ok 1 10 0", b"ok 1 11 2147483647", b"ok 1 12 3", b"ok 1 2147483647 0",
                                  b"ok 10 3 4", b"ok 2 1 1"]
    assert got[len(dc.GOOD):len(dc.GOOD) + len(dc.BAD)] == [b"bad"] * len(dc.BAD)


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_last_line_without_lf(tool, tmp_path):
    lines = [b"a\t1\t2", b"b\t3\t4"]
    assert dump(tool, tmp_path, lines, final_lf=False) == expected(lines)


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_random_lines(tool, tmp_path):
    lines = dc.random_lines(synth.rng_for(11), 2000)
    want = expected(lines)
    assert 400 < want.count(b"bad") < 1600
    if lines[-1] == b"":
        lines.append(b"z\t1\t1"); want.append(b"ok 1 1 1")
    assert dump(tool, tmp_path, lines) == want
