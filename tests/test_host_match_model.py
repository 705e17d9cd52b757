"""The three CPU statements of `matching` must agree before any of them judges the device (tests/test_gpu_match_abi.py): the
model of tests/match_cases.py (every documented field of every component), tests/match_bruteforce.py and
oracle/match_oracle.cpp (both: the text the executable writes).  The model's components are formatted by the executable's
rules -- later-round singletons dropped, repeats dropped, `self` records under -s, cycles opened at open_at under -b -- and
compared as text, on every case family and on the hypothesis strategy of tests/test_match_second_opinion.py.  CPU only."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings

from oracle import binding as orc
from tests import match_cases as mc
from tests.match_bruteforce import decompose
from tests.test_match_glue import numpy_arcs
from tests.test_match_second_opinion import graph_text, tiny_graphs

FLAGS = [(False, False, False), (True, False, False), (False, True, False), (True, True, True), (False, False, True)]      # -s, -b, --aggressive


def _three_ways(tmp_path, graph, iterations, flags, names=None, cap=1 << 20):
    copies, juncs = graph
    self_loops, break_cycles, aggressive = flags
    names = names or mc.names_for(len(copies))
    recs = mc.junc_records(juncs)
    got = mc.text(mc.model(graph, iterations, aggressive), names, self_loops, break_cycles)
    assert got == decompose(names, copies, recs, iterations, aggressive, self_loops, break_cycles)
    path = str(tmp_path / "g.txt")
    open(path, "w").write(graph_text(names, copies, recs))
    lin, cyc = orc.match_run(path, None, iterations, self_loops=self_loops, break_cycles=break_cycles, aggressive=aggressive, cap=cap)
    assert got == (lin.decode(), cyc.decode())
    return got


@pytest.mark.parametrize("family", [f for f in mc.FAMILIES if f != "staircases"])
def test_model_equals_bruteforce_and_oracle_on_the_family(tmp_path, family):
    graph = mc.FAMILIES[family]()
    for flags in FLAGS:
        lin, cyc = _three_ways(tmp_path, graph, 10, flags, cap=8 << 20)
        assert lin


@pytest.mark.parametrize("iterations", mc.STAIRCASE_ITERATIONS)
def test_model_equals_bruteforce_and_oracle_on_the_staircases(tmp_path, iterations):
    for graph in mc.staircase_graphs() + [mc.FAMILIES["staircases"]()]:
        for flags in FLAGS:
            _three_ways(tmp_path, graph, iterations, flags)


def test_every_family_produces_what_it_exists_for():
    for family, needs in mc.NEEDS.items():
        c = mc.census(family)
        assert all(c[k] > 0 for k in needs), (family, c)


def test_staircase_loses_one_segment_per_round_and_the_extra_round_is_numbered_after_the_iterations():
    """the premise of the round-group tests: k rounds of one path each, and `iter` of the aggressive round is `iterations`
    although the graph died long before"""
    comps = mc.model(mc.staircase(6), 12)
    assert [(c[0], c[1], c[3]) for c in comps] == [(mc.PATH, t, [2 * s for s in range(t, 6)]) for t in range(6)]
    comps = mc.model(mc.staircase(4), 12, aggressive=True)
    assert [c[1] for c in comps] == [0, 1, 2, 3, 12] and comps[-1][3] == [0, 2, 4, 6]


def test_path_backed_arcs_rank_first_among_equal_weights(tmp_path):
    """the one extra key of matching -l / palace_stage04_match(use_paths): the model with `backed` against the oracle reading
    the same contigs.paths (the brute force has no paths)"""
    copies, juncs, lines = mc.backed_case()
    names, backed = mc.names_for(len(copies)), mc.backed_arcs(lines)
    text = ["NODE_1_length_9_cov_1\n" + ",".join("%d%s" % ((t >> 1) + 1, "+-"[t & 1]) for t in toks) + "\n" for toks in lines]
    open(tmp_path / "g.txt", "w").write(graph_text(names, copies, mc.junc_records(juncs)))
    open(tmp_path / "p.txt", "w").write("".join(text))
    for self_loops, break_cycles, aggressive in FLAGS:
        got = mc.text(mc.model((copies, juncs), 10, aggressive, backed), names, self_loops, break_cycles)
        lin, cyc = orc.match_run(str(tmp_path / "g.txt"), str(tmp_path / "p.txt"), 10, self_loops=self_loops, break_cycles=break_cycles, aggressive=aggressive,
                                 cap=1 << 20)
        assert got == (lin.decode(), cyc.decode())
    assert mc.rank_arcs(juncs, backed) != mc.rank_arcs(juncs + [(u, v, 0) for u, v in backed])      # the key decides somewhere


@settings(max_examples=250, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True)
@given(tiny_graphs())
def test_model_equals_bruteforce_and_oracle_on_hypothesis_graphs(tmp_path_factory, g):
    names, copies, recs, (self_loops, break_cycles, aggressive) = g
    juncs = [(2 * l + (a == "-"), 2 * r + (b == "-"), w) for l, a, r, b, w in recs]
    _three_ways(tmp_path_factory.mktemp("m"), (copies, juncs), 10, (self_loops, break_cycles, aggressive), names)


def _edges(juncs):
    from palace_amd import capi
    e = np.zeros(len(juncs), capi.EDGE_DTYPE)
    for i, (u, v, w) in enumerate(juncs):
        e[i]["left"], e[i]["oL"], e[i]["right"], e[i]["oR"] = u >> 1, u & 1, v >> 1, v & 1
        e[i]["counts"] = (w // 2, 0, w - w // 2, 0)
    return e


@pytest.mark.parametrize("family", list(mc.FAMILIES) + ["repeated"])
def test_rank_arcs_equals_the_numpy_statement(family):
    if family == "repeated":                                       # the same junction several times, as arc and as conjugate: weights add up
        rng = np.random.Generator(np.random.PCG64(5))
        copies = [1] * 6
        juncs = [(int(rng.integers(0, 12)), int(rng.integers(0, 12)), int(rng.integers(1, 4))) for _ in range(400)]
    else:
        copies, juncs = mc.FAMILIES[family]()
    _, u, v, w = numpy_arcs(np.array(copies, np.int32), _edges(juncs), 0)
    assert mc.rank_arcs(juncs) == list(zip(u.tolist(), v.tolist(), w.tolist()))
