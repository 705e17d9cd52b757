"""The count table's state record (csrc/eref_table_state.hpp) on a CPU: the stand-alone `eref_state_selftest`, as built and under
ASan + UBSan, reaches every state of tests/eref_state_cases.py by the named transitions and prints every guard's answer; the answers must
be those of the table of expectations.  (The same matrix through the C ABI on a device: tests/test_gpu_eref_state.py.)"""
import os
import subprocess

import pytest

from tests import eref_state_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
NAMES = ("eref_state_selftest", "eref_state_selftest_asan")
KEYS = 3 * 36000                                         # what the selftest's count adds


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in NAMES], check=True, stdout=subprocess.DEVNULL)


def guards(tool):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([os.path.join(BIN, tool)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]
    out = {}
    for line in p.stdout.decode().splitlines():
        name, *pairs = line.split()
        assert name not in out
        out[name] = {k: int(v) for k, v in (pair.split("=") for pair in pairs)}
    return out


@pytest.mark.parametrize("tool", NAMES, ids=["plain", "asan"])
def test_every_state_answers_as_the_table_says(tool):
    g = guards(tool)
    assert set(cases.STATES) <= set(g)
    for call, accepting in cases.ACCEPTED.items():
        for state in cases.STATES:
            assert cases.accepted_by_guards(call, state, g[state]) == (state in accepting), (call, state)
    for state in cases.STATES:
        assert g[state]["first_plane"] == cases.FIRST_PLANE_TO_CLEAR[state], state
        assert g[state]["clean"] == (state in ("Z", "C0")), state               # after a partial count of no reads the planes are still zero
    # what the indexed scan starts from: nothing, channel 0, or every entry set (the sentinels in place only when the count put them there)
    assert [g[s]["hit_sets_ix"] for s in cases.STATES] == [0, 0, 0, 0, 1, 15, 0, 0, 15]
    assert [g[s]["sentinels_ix"] for s in cases.STATES] == [0, 0, 0, 0, 0, 1, 0, 0, 0]
    assert not any(g[s]["hit_sets_other"] for s in g)
    assert [g[s]["keys"] for s in cases.STATES] == [0, KEYS, -1, KEYS, KEYS, KEYS, KEYS, 0, KEYS]
    assert g["new"]["clean"] == 0 and g["new"]["takes_counts"] == 1 and g["allocated"]["clean"] == 1      # planes not yet allocated: nothing known


@pytest.mark.parametrize("tool", NAMES, ids=["plain", "asan"])
def test_every_write_of_the_planes_drops_the_fused_record(tool):
    g = guards(tool)
    assert g["T0"]["hit_sets_ix"] == 1
    for after in ("count_started", "counted_direct", "counted_plain", "merged", "unpacked", "counted_final", "counted_partial", "unknown", "reset"):
        assert g["T0+" + after]["hit_sets_ix"] == 0, after
    # the merge after a partial count of no reads whose hit bits were declared whole: the scan probes the merged planes for itself
    assert g["C0+whole"]["hit_sets_ix"] == 15 and g["C0+whole"]["takes_counts"] == 1 and g["C0+whole"]["clean"] == 1
    assert g["C0+whole+merged"]["hit_sets_ix"] == 0 and g["C0+whole+merged"]["planes_readable"] == 1 and g["C0+whole+merged"]["keys"] == -1
    # an index that goes away takes its record along, another one's leaves it; a re-pointed count block is no longer this context's
    assert g["T0+other_index_gone"] == g["T0"] and g["T0+index_gone"]["hit_sets_ix"] == 0 and g["T0+detached"]["hit_sets_ix"] == 0
    assert g["C"]["counts_in_block"] == 1 and g["C+block_detached"]["counts_in_block"] == 0
    # the sparse unpack keeps the key count (the scan's pruning order goes by it) and a top-only table top-only
    assert g["T0+unpacked"]["keys"] == KEYS and g["T0+unpacked"]["takes_counts"] == 0 and g["T0+unpacked"]["first_plane"] == 2
    assert g["Z+unpacked"]["keys"] == 0 and g["Z+unpacked"]["clean"] == 0 and g["Z+unpacked"]["takes_counts"] == 1
    assert g["T0+merged"]["keys"] == -1 and g["T0+merged"]["sparse"] == 0 and g["P"]["sparse"] == 1
