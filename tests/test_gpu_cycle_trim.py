"""palace_cycle_trim (csrc/final_fasta.hip) at the C ABI, on integers only, against the LITERAL restatement of the cycle test in
tests/final_fa_cases.py (every interval, every sum afresh); the one path too long for that against the pruned restatement, which
tests/test_host_final_fa_rules.py holds to the literal one."""
import numpy as np
import pytest

from palace_amd import capi
from tests import final_fa_cases as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def run(ctx, paths, arcs, thr, mn, decide=fc.cycle_interval):
    """paths: [(node, base, length)] -> the device's (first, last) per path, checked against `decide`"""
    node = np.concatenate([np.asarray(p[0], np.int32) for p in paths] + [np.zeros(0, np.int32)])
    base = np.concatenate([np.asarray(p[1], np.int32) for p in paths] + [np.zeros(0, np.int32)])
    length = np.concatenate([np.asarray(p[2], np.int64) for p in paths] + [np.zeros(0, np.int64)])
    path_off = np.zeros(len(paths) + 1, np.int64)
    np.cumsum([len(p[0]) for p in paths], out=path_off[1:])
    keys = np.array([(a << 32) | b for a, b in arcs], np.uint64)
    first, last, intact = capi.cycle_trim(ctx, node, base, length, path_off, keys, thr, mn)
    assert intact, "entries outside d_first / d_last were written"
    got = [(int(a), int(b)) for a, b in zip(first, last)]
    arc_set = set(arcs)
    want = [decide([int(v) for v in p[0]], [int(v) for v in p[1]], [int(v) for v in p[2]], arc_set, thr, mn) for p in paths]
    assert got == want, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    return got


def random_path(rng, L, n_base=None, lens=(0, 1, 2, 3, 5, 8, 50)):
    n_base = n_base or max(1, L // 3)
    base_len = rng.choice(lens, size=n_base)
    base = rng.integers(0, n_base, size=L)
    return 2 * base + rng.integers(0, 2, size=L), base, base_len[base] if L else np.zeros(0, np.int64)


def random_arcs(rng, n, n_nodes):
    return [(int(a), int(b)) for a, b in rng.integers(0, n_nodes, size=(n, 2))]


@pytest.mark.parametrize("L", [0, 1, 2, 63, 64, 65, 129, 300])
def test_one_path_of_every_length(ctx, L):
    rng = np.random.default_rng(100 + L)
    n_base = min(max(1, L // 3), 10)
    path = random_path(rng, L, n_base)
    uniq = int(sum({int(b): int(l) for b, l in zip(path[1], path[2])}.values()))
    hits = 0
    for n_arcs, thr, mn in ((0, 60, 0), (1, 60, 0), (5000, 0, 0), (5000, 7, int(0.6 * uniq)), (5000, 60, uniq), (5000, 10 ** 9, 1)):
        arcs = [a for a in random_arcs(rng, n_arcs, 2 * n_base) if (a[0] * 7 + a[1]) % 3]      # (5 000 draws from few pairs: duplicate keys; a third of the pairs absent)
        if n_arcs == 1 and L:
            arcs = [(int(path[0][-1]), int(path[0][0]))]
        hits += run(ctx, [path], arcs, thr, mn)[0][0] >= 0
    assert hits >= (2 if L >= 63 else 1 if L else 0)                             # (not vacuous: the single closing arc, and with no threshold some arc)


def test_no_paths(ctx):
    assert run(ctx, [], [(0, 0)], 300, 0) == []


def test_2500_paths_of_mixed_lengths(ctx):
    rng = np.random.default_rng(7)
    lengths = [int(rng.integers(0, 41)) for _ in range(2500)]
    for k, L in ((3, 63), (700, 64), (701, 65), (1900, 129), (2499, 130), (0, 0), (1, 0), (2498, 0)):
        lengths[k] = L
    n_base = 12
    paths = [random_path(rng, L, n_base) for L in lengths]
    arcs = random_arcs(rng, 5000, 2 * n_base)
    arcs = [a for a in arcs if (a[0] * 7 + a[1]) % 3]                           # (a third of the pairs absent)
    got = run(ctx, paths, arcs, 9, 25)
    n_cyc = sum(1 for g in got if g[0] >= 0)
    assert 300 < n_cyc < 2200 and sum(1 for g, L in zip(got, lengths) if g[0] > 0 or 0 <= g[1] < L - 1) > 100      # cycles, trimmed ones among them


def test_a_path_of_5000_whose_lengths_all_exceed_the_threshold(ctx):
    rng = np.random.default_rng(8)
    L, n_base = 5000, 900
    base_len = rng.integers(301, 5000, size=n_base)
    base = rng.integers(0, n_base, size=L)
    path = (2 * base + rng.integers(0, 2, size=L), base, base_len[base])
    uniq = int(base_len[np.unique(base)].sum())
    closing = (int(path[0][-1]), int(path[0][0]))
    arcs = random_arcs(rng, 5000, 2 * n_base) + [closing]
    assert run(ctx, [path], arcs, 300, uniq, fc.cycle_interval_pruned) == [(0, L - 1)]
    assert run(ctx, [path], arcs, 300, uniq + 1, fc.cycle_interval_pruned) == [(-1, -1)]
    assert run(ctx, [path], [a for a in arcs if a != closing], 300, uniq, fc.cycle_interval_pruned) == [(-1, -1)]


# ---- planted edges ----------------------------------------------------------------------------------------------------------------

def plain(lens, ids=None):
    ids = list(range(len(lens))) if ids is None else ids
    return ids, ids, lens


def test_trimmed_at_the_threshold_and_one_above(ctx):
    p = plain([120, 9000, 9000, 180])
    assert run(ctx, [p], [(2, 1)], 300, 10000) == [(1, 2)]
    assert run(ctx, [p], [(2, 1)], 299, 10000) == [(-1, -1)]
    q = plain([120, 9000, 9000, 181])                                            # threshold + 1
    assert run(ctx, [q], [(2, 1)], 300, 10000) == [(-1, -1)]


def test_unique_length_at_the_minimum_and_one_below(ctx):
    assert run(ctx, [plain([9999, 1])], [(1, 0)], 300, 10000) == [(0, 1)]
    assert run(ctx, [plain([9998, 1])], [(1, 0)], 300, 10000) == [(-1, -1)]
    assert run(ctx, [plain([9999, 1])], [(1, 0)], 300, 10001) == [(-1, -1)]


def test_a_base_in_both_orientations_repeated_inside_and_outside_the_interval(ctx):
    # tokens 4+ 1+ 1- 2+ 1+ 4-: base 1 three times inside [1, 4], base 4 on both sides outside it; nodes are 2 * base + strand
    node, base = [8, 2, 3, 4, 2, 9], [4, 1, 1, 2, 1, 4]
    lens = [100, 3000, 3000, 500, 3000, 100]
    arcs = [(2, 2)]                                                              # 1+ -> 1+ closes [1, 4] and [1, 1], [4, 4]
    assert run(ctx, [(node, base, lens)], arcs, 200, 3500) == [(1, 4)]           # distinct bases 1 and 2: 3500, not 9500
    assert run(ctx, [(node, base, lens)], arcs, 200, 3501) == [(-1, -1)]
    assert run(ctx, [(node, base, lens)], [(9, 8)], 0, 3600) == [(0, 5)]          # whole path: bases 4, 1, 2 = 3600
    assert run(ctx, [(node, base, lens)], [(9, 8)], 0, 3601) == [(-1, -1)]
    assert run(ctx, [(node, base, lens)], [(3, 2)], 10 ** 6, 3000) == [(1, 2)]           # 1- -> 1+ closes [1, 2], which trims 3700
    assert run(ctx, [(node, base, lens)], [(3, 2), (2, 3)], 10 ** 6, 3000) == [(2, 4)]   # 1+ -> 1- closes [2, 4], which trims 3200
    assert run(ctx, [(node, base, lens)], [(3, 2), (2, 3)], 10 ** 6, 3501) == [(-1, -1)]


def test_an_arc_present_only_as_a_conjugate(ctx):
    # the host adds both arcs of a JUNC line; here only the conjugate's key is given: it is an arc like any other, the other direction is none
    p = ([5, 2], [2, 1], [6000, 6000])
    assert run(ctx, [p], [(2, 5)], 300, 10000) == [(0, 1)]
    assert run(ctx, [p], [(5, 2)], 300, 10000) == [(-1, -1)]


def test_the_tie_of_front_trim_and_back_trim_keeps_the_first_interval(ctx):
    for L in (4, 70):
        lens = [100] + [7000] * (L - 2) + [100]
        p = plain(lens)
        assert run(ctx, [p], [(L - 1, 1), (L - 2, 0)], 300, 10000) == [(0, L - 2)]
        assert run(ctx, [p], [(L - 1, 1)], 300, 10000) == [(1, L - 1)]


def test_zero_length_nodes_make_every_interval_a_candidate(ctx):
    L = 65
    p = plain([0] * L)
    assert run(ctx, [p], [(L - 1, L - 1)], 0, 0) == [(L - 1, L - 1)]
    assert run(ctx, [p], [(40, 3), (64, 64), (3, 3)], 0, 0) == [(3, 3)]           # all trimmed 0: the first in (i, j) order
    assert run(ctx, [p], [(40, 3), (64, 64)], 0, 0) == [(3, 40)]
    assert run(ctx, [p], [(40, 3)], 0, 1) == [(-1, -1)]
    rng = np.random.default_rng(9)
    node = rng.integers(0, 6, size=L)
    run(ctx, [(node, node // 2, [0] * L)], [(5, 0), (3, 4), (1, 1)], 0, 0)


def test_threshold_zero_and_negative(ctx):
    p = plain([5, 5, 5])
    assert run(ctx, [p], [(2, 0), (1, 1)], 0, 0) == [(0, 2)]
    assert run(ctx, [p], [(1, 1)], 0, 0) == [(-1, -1)]
    assert run(ctx, [p], [(2, 0), (1, 1)], -1, 0) == [(-1, -1)]
    assert run(ctx, [plain([0, 0])], [(0, 0), (1, 0)], -1, 0) == [(-1, -1)]
    assert run(ctx, [p], [(2, 0)], -(1 << 62), 0) == [(-1, -1)]


def test_a_self_arc_on_a_one_token_path(ctx):
    assert run(ctx, [plain([12000], [7])], [(7, 7)], 300, 10000) == [(0, 0)]
    assert run(ctx, [plain([12000], [7])], [(7, 6), (6, 7)], 300, 10000) == [(-1, -1)]
    assert run(ctx, [plain([9000], [7])], [(7, 7)], 300, 10000) == [(-1, -1)]
