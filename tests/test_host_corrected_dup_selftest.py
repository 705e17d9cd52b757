"""host/corrected_dup_rules.hpp -- the token grammar, the list surgery of one path, the double arithmetic, the order of the output --
driven by the stand-alone `corrected_dup_selftest`, as built and under ASan + UBSan (nothing preloaded, no device): every case of
tests/golden/corrected_dup_cases.npz must come out as the reference's script wrote it, the device's four answers being brute force
inside the program."""
import os
import subprocess

import numpy as np
import pytest

from tests import corrected_dup_cases as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = ["corrected_dup_selftest", "corrected_dup_selftest_asan"]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in TOOLS], check=True, stdout=subprocess.DEVNULL)


def case_text(case):
    fai, depth = cd.parse_inputs(case)
    row = {n: k for k, n in enumerate(fai)}

    def path(tokens):
        return f"{len(tokens)} " + " ".join(str(row[t[:-1]] << 1 | (t[-1] == "-")) for t in tokens)

    cycles = [r.split() for r in case["cycle"].decode().splitlines()]
    finals = [r.split() for r in case["final"].decode().splitlines() if r.split()]
    cuts = [r.strip().split(":") for r in case["before_cut"].decode().splitlines()]
    text = [f"fai {len(fai)}"] + [f"{n} {ln} {depth.get(n, (0, 0))[0]} {depth.get(n, (0, 0))[1]}" for n, ln in fai.items()]
    text += [f"cycles {len(cycles)}"] + [path(c) for c in cycles] + [f"finals {len(finals)}"] + [path(f) for f in finals]
    text += [f"cuts {len(cuts)}"] + [path(k.split()) + " " + path(v.split()) for k, v in cuts] + [f"min_len {case['min_len']}"]
    return ("\n".join(text) + "\n").encode()


@pytest.mark.parametrize("tool", TOOLS)
def test_every_golden_case(tool):
    golden = np.load(os.path.join(ROOT, "tests", "golden", "corrected_dup_cases.npz"))
    cases = cd.golden_inputs()
    names = sorted({k.split("__")[0] for k in golden.files})
    assert len(names) >= 60
    for name in names:
        p = subprocess.run([os.path.join(BIN, tool)], input=case_text(cases[name]), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 0 and p.stderr == b"", (name, p.returncode, p.stderr[-400:])
        assert p.stdout == golden[name + "__out"].tobytes() + b"--\n" + golden[name + "__stdout"].tobytes(), name


@pytest.mark.parametrize("tool", TOOLS)
def test_the_token_grammar(tool):
    e = cd.edge(1, 5, "2.0")
    words = [e + "+", "ctg-", e, "a+b+", "a-b+", "a:b+", "x" + e + "+", "", "+", "EDGE_1_length_5_cov_+", "EDGE_" + e + "-", "xEDGE_1_length_+"]
    want = ["ok", "ok", "does not end in '+' or '-'", "holds a '+', '-' or ':' inside", "holds a '+', '-' or ':' inside", "holds a '+', '-' or ':' inside",
            "matches the EDGE pattern in part only", "does not end in '+' or '-'", "ok", "ok", "matches the EDGE pattern in part only", "ok"]
    p = subprocess.run([os.path.join(BIN, tool), "words"], input=("\n".join(words) + "\n").encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and p.stderr == b""
    assert p.stdout.decode().splitlines() == want
