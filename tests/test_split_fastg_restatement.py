"""The Python restatement of split_fastg (tests/split_fastg_cases.py) against what the reference's script wrote
(tests/golden/split_fastg_cases.npz, made by tests/golden/make_split_fastg_golden.py), and its verdicts on hand-made faults.  CPU."""
import os

import numpy as np
import pytest

from tests import split_fastg_cases as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_fastg_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_inputs_are_the_builders(golden):
    cases = sc.golden_inputs()
    assert sorted(k[:-4] for k in golden.files if k.endswith("__in")) == sorted(cases)
    for name, text in cases.items():
        assert golden[name + "__in"].tobytes() == text, name
    assert os.path.getsize(GOLDEN) < 300 * 1024


@pytest.mark.parametrize("name", sorted(sc.golden_inputs()))
def test_restatement_equals_the_reference(golden, name):
    text, want = golden[name + "__in"].tobytes(), golden[name + "__out"].tobytes()
    assert sc.verdict(text) == (0, 0)
    assert sc.split_fastg(text) == want


def test_golden_covers_what_it_should(golden):
    out = {k[:-5]: golden[k].tobytes() for k in golden.files if k.endswith("__out")}
    assert out["quirks"].startswith(b">EDGE_3_length_4_cov_\nACGT\n>EDGE_4\tx\nACG\n>\nGT\n>'\nAC\n")
    assert out["three_of_one_name"] == b">E_1\nAAAA\n>E_2\nCC\n"
    assert out["primed_first_lower"] == b">EDGE_1_length_8_cov_2\nACGTACGT\n>EDGE_2_length_4_cov_1\nacNn\n"
    assert b">E_2\n\n" in out["empty_sequences"] and out["crlf_small"].count(b"\r") == 0
    lens = sorted(len(s) for s in out["spades60"].split(b"\n")[1::2])
    assert lens == sorted(sc.LENGTHS)


@pytest.mark.parametrize("name", sorted(sc.fault_cases()))
def test_faults(name):
    text, code, line = sc.fault_cases()[name]
    assert sc.verdict(text) == (code, line)
    with pytest.raises(sc.FastgError) as e:
        sc.split_fastg(text)
    assert (e.value.code, e.value.line) == (code, line)


def test_hand_checks():
    sc.hand_checks()
