"""The rules of make_final_fa on the host: the Python restatement of tests/final_fa_cases.py against what the reference's script
itself wrote (tests/golden/final_fa_cases.npz; PINNED: graph rules, cycle decision, order, numbering, separators, headers, stderr;
UNPINNED: the FASTA reader and the complement table, which are a stand-in's where the golden file is made), the pruned form of the
cycle test against the literal one, and host/final_tokens.hpp -- driven by the stand-alone `final_tokens_selftest`, as built and
under ASan + UBSan, nothing preloaded -- against the restatement's tokeniser."""
import os
import subprocess

import numpy as np
import pytest

from tests import final_fa_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = [os.path.join(BIN, t) for t in ("final_tokens_selftest", "final_tokens_selftest_asan")]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in ("final_tokens_selftest", "final_tokens_selftest_asan")],
                   check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "final_fa_cases.npz"))


def test_restatement_against_hand_worked_cases():
    fc.hand_checks()


def test_restatement_equals_the_reference_on_every_golden_case(golden):
    cases = fc.golden_inputs()
    assert len(cases) >= 15 and {k.split("__")[0] for k in golden.files} == set(cases)
    n_cycle = n_linear = n_warn = 0
    for name, (paths, graph, fasta, prefix, words) in cases.items():
        for key, val in (("paths", paths), ("graph", graph), ("fasta", fasta), ("prefix", prefix), ("args", b"\0".join(words))):
            assert golden[f"{name}__{key}"].tobytes() == val, (name, key)          # the inputs the reference saw are the catalogue's
        thr, mn = fc.options_of(words)
        out, err = fc.final_fa(paths, graph, fasta, prefix, b"asm.fasta", b"out.fasta", thr, mn)
        assert out == golden[name + "__out"].tobytes(), name
        assert err == golden[name + "__err"].tobytes(), name
        n_cycle, n_linear, n_warn = n_cycle + out.count(b"_cycle\n"), n_linear + out.count(b"_linear\n"), n_warn + err.count(b"Warning: ")
    assert n_cycle > 30 and n_linear > 100 and n_warn > 100


def random_integer_path(rng, max_len=40):
    """one path as integers, small enough alphabets that arcs, repeats and ties are common -> (node, base, length, arcs, threshold, minimum)"""
    n_base = int(rng.integers(1, 9))
    base_len = rng.choice([0, 0, 1, 2, 3, 5, 8, 50], size=n_base)
    L = int(rng.integers(0, max_len + 1))
    base = rng.integers(0, n_base, size=L)
    node = 2 * base + rng.integers(0, 2, size=L)
    n_arcs = int(rng.integers(0, 4 * n_base + 1))
    arcs = {(int(a), int(b)) for a, b in rng.integers(0, 2 * n_base, size=(n_arcs, 2))}
    thr = int(rng.choice([-1, 0, 1, 3, 10, 60, 10 ** 6]))
    mn = int(rng.choice([0, 1, 4, 9, 30, 120]))
    return [int(v) for v in node], [int(v) for v in base], [int(base_len[b]) for b in base], arcs, thr, mn


def test_pruned_cycle_test_equals_the_literal_one():
    rng = np.random.default_rng(77)
    cycles = trimmed = 0
    for _ in range(2500):
        case = random_integer_path(rng)
        want = fc.cycle_interval(*case)
        assert fc.cycle_interval_pruned(*case) == want, case
        cycles += want[0] >= 0
        trimmed += want[0] > 0 or (want[0] == 0 and want[1] < len(case[0]) - 1)
    assert cycles > 500 and trimmed > 100


def dump(tool, tmp_path, mode, text):
    path = tmp_path / "input.txt"
    path.write_bytes(text)
    p = subprocess.run([tool, mode, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]               # (a sanitizer report goes to stderr and ends the run)
    return p.stdout.split(b"\n")[:-1]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_tokeniser_over_the_catalogue_and_its_faulty_counterparts(tool, tmp_path):
    for name, (paths, graph, _, _, _) in fc.golden_inputs().items():
        assert dump(tool, tmp_path, "paths", paths) == fc.dump_paths(paths), name
        assert dump(tool, tmp_path, "graph", graph) == fc.dump_graph(graph), name
    for name, (which, text, line, reason) in fc.faulty_inputs().items():
        want = [b"F %d %s" % (line, reason)]
        assert (fc.dump_paths if which == "paths" else fc.dump_graph)(text) == want, name
        assert dump(tool, tmp_path, which, text) == want, name
    for text in fc.TOKEN_HAND:
        assert dump(tool, tmp_path, "paths", text) == fc.dump_paths(text), text
        assert dump(tool, tmp_path, "graph", text) == fc.dump_graph(text), text
    assert fc.dump_paths(b"reflength_3ref-ref\n") == [b"L 1 1", b"T 7265666c656e6774685f337265662d726566 3 7265666c656e6774685f337265662d726566 6c656e6774685f332d"]
    assert fc.dump_graph(b"JUNC a_length_1 + b_length_2 - 7\n") == [b"A 615f6c656e6774685f312b 1 625f6c656e6774685f322d 2", b"A 625f6c656e6774685f322b 2 615f6c656e6774685f312d 1"]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_tokeniser_on_random_lines(tool, tmp_path):
    rng = np.random.default_rng(78)
    words = [b"JUNC", b"JUNCx", b"+", b"-", b"a_length_12", b"b_length_0+", b"length_7-", b"c_length_5+-", b"refd_length_3ref+", b"wall", b"x", b"length_", b" ", b"\t",
             b"  ", b"\r"]
    def line():
        return b"".join(words[int(k)] + (b" ", b"\t", b"")[int(rng.integers(0, 3))] for k in rng.integers(0, len(words), size=int(rng.integers(0, 9))))
    good = [w for w in words if w not in (b"x", b"length_", b"\r", b"wall")]
    def good_line():
        return b" ".join(good[int(k)] for k in rng.integers(0, len(good), size=int(rng.integers(0, 9))))
    for make, n in ((line, 40), (good_line, 400)):
        for text in (b"\n".join(make() for _ in range(n)) + b"\n", b"\r\n".join(make() for _ in range(n))):
            assert dump(tool, tmp_path, "paths", text) == fc.dump_paths(text)
            assert dump(tool, tmp_path, "graph", text) == fc.dump_graph(text)
