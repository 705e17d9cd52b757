"""host/path_tokens.hpp -- the lines and tokens of a paths file as make_fa_from_path reads them -- driven by the stand-alone
`path_tokens_selftest`, as built and under ASan + UBSan, against the Python restatement of tests/path_fasta_cases.py; and the
executable's behaviour where no device is visible or the command line is wrong."""
import os
import subprocess

import numpy as np
import pytest

from palace_amd import synth
from tests import path_fasta_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = [os.path.join(BIN, t) for t in ("path_tokens_selftest", "path_tokens_selftest_asan")]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in ("path_tokens_selftest", "path_tokens_selftest_asan", "make_fa_from_path")],
                   check=True, stdout=subprocess.DEVNULL)


def hexed(b):
    return b.hex().encode() if b else b"-"


def expected(paths):
    out = []
    for idx, tokens in pc.path_lines(paths):
        out.append(b"L %d %d" % (idx, len(tokens)))
        out += [b"T " + hexed(t) + b" " + hexed(pc.clean(t)) for t in tokens]
    return out


def dump(tool, tmp_path, paths):
    path = tmp_path / "paths.txt"
    path.write_bytes(paths)
    p = subprocess.run([tool, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]
    return p.stdout.split(b"\n")[:-1]


HAND = [pc.CHAIN_PATHS, pc.CHAIN_PATHS + b"\n", b"", b"\n", b"\n\n", b"a", b"a+\tb-", b"\t\t\n", b"a\t\tb\n", b"iter\nself\niterate+\tx\n itera+\n",
        b" \x0b\x0c a+ \x0c\r\n", b"a \x0b+\tb\r\t\rc\n", b"x\t+\t-\n", b"A B\tC  D \t E\n", b"\r\n\r\n", b"a+\r\nb-\r\n", b"\ta+\n", b"a+\t \n"]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_hand_cases(tool, tmp_path):
    for paths in HAND:
        assert dump(tool, tmp_path, paths) == expected(paths), paths
    assert expected(b"a \x0b+\tb\r\t\rc\n") == [b"L 0 3", b"T 61200b2b 610b2b", b"T 620d 62", b"T 0d63 63"]
    assert expected(b"a\t\tb\n") == [b"L 0 3", b"T 61 61", b"T - -", b"T 62 62"]
    assert expected(b"iter\nself\niterate+\tx\n itera+\n") == [b"L 3 1", b"T 69746572612b 69746572612b"]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_random_lines(tool, tmp_path):
    rng = synth.rng_for(41)
    alphabet = np.frombuffer(b"\t \r+-_a1", np.uint8)
    lines = [alphabet[rng.integers(0, 8, size=int(rng.integers(0, 24)))].tobytes() for _ in range(2000)]
    for text in (b"\n".join(lines) + b"\n", b"\n".join(lines + [b"a1+\t-"])):
        want = expected(text)
        assert 1500 < sum(1 for l in want if l.startswith(b"L")) and any(l == b"T - -" for l in want)
        assert dump(tool, tmp_path, text) == want


def test_executable_without_a_device_or_with_a_wrong_command_line(tmp_path):
    tool = os.path.join(BIN, "make_fa_from_path")
    (tmp_path / "asm.fa").write_bytes(b">a\nACGT\n")
    (tmp_path / "p.txt").write_bytes(b"a+\n")
    out = tmp_path / "out.fa"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    p = subprocess.run([tool, str(tmp_path / "asm.fa"), str(tmp_path / "p.txt"), str(out), "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode != 0 and p.stderr.startswith(b"make_fa_from_path:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1, p.stderr
    assert not out.exists()
    for args in ([], [str(tmp_path / "asm.fa"), str(tmp_path / "p.txt"), str(out)], [str(tmp_path / "asm.fa"), str(tmp_path / "p.txt"), str(out), "0", "extra"],
                 ["--batch", str(tmp_path / "p.txt")]):
        p = subprocess.run([tool] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert p.returncode != 0 and p.stderr.startswith(b"Usage: make_fa_from_path") and p.stdout == b"", (args, p.stderr)
        assert not out.exists()


def test_restatement_against_hand_written_files():
    pc.hand_checks()
