"""The rules of corrected_dup on the host: the Python model of tests/corrected_dup_cases.py against what the reference's script itself
wrote (tests/golden/corrected_dup_cases.npz: every stored case ran under four hash seeds with identical bytes; PINNED: reformat,
units, copies by depth, push-back, similarity, before_cut, the base-set skip, the quota, the length filter; UNPINNED: samtools'
depth rules, which are a stand-in's where the golden file is made), the order of the units -- DECLARED, not pinned: the script
leaves it to a set of strings -- on two hand cases, and the brute-force form of each kernel contract against the model's own use
of it."""
import os

import numpy as np
import pytest

from tests import corrected_dup_cases as cd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "corrected_dup_cases.npz"))


def test_model_equals_the_reference_on_every_golden_case(golden):
    cases = cd.golden_inputs()
    stored = sorted({k.split("__")[0] for k in golden.files})
    assert len(stored) >= 60 and set(stored) <= set(cases) and 10 * (len(cases) - len(stored)) <= len(cases)
    seen, rewritten = set(), 0
    for name in stored:
        case = cases[name]
        for key in ("fai", "cycle", "final", "before_cut", "depth"):
            assert golden[f"{name}__{key}"].tobytes() == case[key], (name, key)              # the inputs the reference saw are the catalogue's
        assert int(golden[name + "__min_len"][0]) == case["min_len"]
        out, stdout = cd.corrected_dup(case, seen)
        assert out == golden[name + "__out"].tobytes(), name
        assert stdout == golden[name + "__stdout"].tobytes(), name
        given = set(case["cycle"].splitlines()) | set(case["final"].splitlines())
        rewritten += any(row not in given for row in out.splitlines())
    assert set(cd.FEATURES) <= seen, sorted(set(cd.FEATURES) - seen)
    assert 2 * rewritten >= len(stored)


def test_units_are_pushed_back_in_discovery_order():
    """DECLARED, not pinned: [b] is found before [c d] (periods ascend), and the other order gives another line"""
    fai = {"b": 100, "c": 300, "d": 450, "e": 50}
    depth = {n: (10 * ln, ln) for n, ln in fai.items()}
    for line, want_units in (("b+ c+ d+ c+ d+ b+ b+ e+ b+", [["b+"], ["c+", "d+"]]),      # a border of 1: b b c d c d b b e
                             ("c+ d+ b+ b+ c+ d+ c+ d+ c+ d+", [["b+"], ["c+", "d+"]])):   # a border of 2: c d c d b b c d c d
        tokens = line.split()
        rotated = cd.reformat(tokens, set())
        assert cd.tandem_units(rotated) == want_units
        first = cd.correct_cycle(tokens, fai, depth, set())
        assert first == cd.correct_cycle(tokens, fai, depth, set(), units=want_units)
        assert first != cd.correct_cycle(tokens, fai, depth, set(), units=want_units[::-1])


def lines_of_cases():
    for case in cd.golden_inputs().values():
        rows = [r.split() for r in case["cycle"].decode().splitlines()]
        yield case, rows, [r.split() for r in case["final"].decode().splitlines() if r.split()]


def test_brute_forces_agree_with_the_models_use_of_them():
    rng = np.random.default_rng(3)
    for p in [[int(t) for t in rng.integers(0, 2, size=n)] for n in (0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129)] + [[1] * 40, [1, 2] * 20 + [1]]:
        assert [tuple(int(x) for x in row) for row in cd.tandem_candidates_np(p)] == cd.tandem_candidates(p)
    n_border = n_skip = n_drop = 0
    for case, cycles, finals in lines_of_cases():
        fai, _ = cd.parse_inputs(case)
        for row in cycles:
            L = cd.border(row)
            n_border += L > 0
            assert cd.reformat(row, set())[:L] == row[len(row) - L:] if L else True
            line = cd.reformat(row, set())
            assert cd.tandem_units(line) == cd.tandem_units(line, [tuple(int(x) for x in c) for c in cd.tandem_candidates_np([hash(t) for t in line])])
        bases = [[cd.base_of(t) for t in row] for row in cycles + finals]
        skip = cd.base_set_in(bases, len(cycles))
        assert [bool(s) for s in skip[len(cycles):]] == [any(set(b) == set(c) for c in bases[:len(cycles)]) for b in bases[len(cycles):]]
        n_skip += int(skip.sum())
        lens = [[fai[cd.base_of(t)] for t in row] for row in cycles + finals]
        rel = cd.length_relation(lens)
        kept = cd.greedy_keep(len(lens), lambda i, j: rel[i, j])
        assert kept == cd.greedy_paths(cycles + finals, fai, set())
        n_drop += len(lens) - len(kept)
    assert n_border > 5 and n_skip > 5 and n_drop > 10
