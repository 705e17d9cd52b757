"""csrc/blast_line.hpp, the grammar of one line of the BLAST table that the kernels of csrc/filter_result.hip compile: driven by the
stand-alone `blast_line_selftest` (its own main, every line in an allocation of exactly its length), as built and under ASan + UBSan
with nothing preloaded, over the catalogue's tables and their malformed counterparts, against the restatement's line reader."""
import os
import subprocess

import numpy as np
import pytest

from tests import filter_result_cases as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
NAMES = ("blast_line_selftest", "blast_line_selftest_asan")
TOOLS = [os.path.join(BIN, t) for t in NAMES]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in NAMES], check=True, stdout=subprocess.DEVNULL)


def dump(tool, tmp_path, text):
    path = tmp_path / "table.txt"
    path.write_bytes(text)
    p = subprocess.run([tool, "lines", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]               # (a sanitizer report goes to stderr and ends the run)
    return p.stdout.split(b"\n")[:-1]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_line_reader_over_the_catalogue_and_its_malformed_counterparts(tool, tmp_path):
    codes = set()
    for text in fr.malformed_tables() + [case[2] for _, case, _, _ in fr.faulty_inputs().values()]:
        want = fr.dump_blast(text)
        assert dump(tool, tmp_path, text) == want, text[:200]
        codes |= {w[:3] for w in want}
    assert codes == {b"E 1", b"E 2", b"E 3", b"E 4"} | {w for w in codes if w.startswith(b"L")} and len(codes) > 5


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_line_reader_on_random_lines(tool, tmp_path):
    rng = np.random.default_rng(91)
    words = [b"q", b"subject_1", b"", b"99", b"100.0", b"7.123456", b"7.1234567", b"1000", b"0", b"1234567890", b"12345678901", b".", b"5.", b".5", b"-1", b"1e2",
             b" 5", b"x\r"]
    def any_line():
        return b"\t".join(words[int(k)] for k in rng.integers(0, len(words), size=int(rng.integers(0, 7))))

    def shaped_line():                                   # names in front, two words where the numbers stand, perhaps more columns
        return b"\t".join([b"q", b"s"] + [words[int(k)] for k in rng.integers(3, len(words), size=int(rng.integers(2, 5)))])
    lines = [(any_line, shaped_line)[k % 2]() for k in range(1500)]
    for text in (b"\n".join(lines) + b"\n", b"\n".join(lines[:50])):
        assert dump(tool, tmp_path, text) == fr.dump_blast(text)
    want = fr.dump_blast(b"\n".join(lines))
    assert sum(w.startswith(b"L") for w in want) > 40 and {w for w in want if w.startswith(b"E")} == {b"E 1", b"E 2", b"E 3", b"E 4"}
