"""The path / cycle decomposition at the C ABI against the exact model of tests/match_cases.py (which tests/test_host_match_model.py
ties to the two other CPU statements): every field include/palace_hip.h documents per component -- off, verts, kind, iter,
open_at, in emission order, repeats included -- element for element, no tolerance.  The graphs are the adversarial families of
match_cases.py, thousands of tiny graphs per device call as one union; the three ways the decomposition ranks arcs
(position alone in palace_match_decompose; one-word and two-word keys in palace_stage04_match) are each run on purpose, and
palace_match_last_run says which one produced the result, so a test of a mode cannot silently stop covering it.
palace_match_greedy is held to a sequential greedy over the arcs in id order."""
import functools

import numpy as np
import pytest

from palace_amd import capi, stage04_io
from tests import match_cases as mc

pytestmark = pytest.mark.gpu
FIELDS = ("off", "verts", "kind", "iter", "open_at")


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def family(name):
    if name == "all":
        return mc.union([family(f) for f in mc.FAMILIES])
    if name == "settling":                                     # everything but the long zig-zags: every round settles in the enqueued iterations
        return mc.union([family(f) for f in mc.FAMILIES if f != "zigzags"] + [mc.zigzag(k) for k in mc.ZIGZAG_ARCS if k <= 8])
    return mc.FAMILIES[name]()


@functools.lru_cache(maxsize=None)
def ranked(name):
    return mc.rank_arcs(family(name)[1])


@functools.lru_cache(maxsize=None)
def expected_and_needed(name, iterations, aggressive):
    copies, needed = family(name)[0], []
    return mc.components(len(copies), copies, ranked(name), iterations, aggressive, needed), needed


def expected(name, iterations, aggressive):
    return expected_and_needed(name, iterations, aggressive)[0]


def arc_arrays(arcs):
    return np.array([a[0] for a in arcs], np.int32), np.array([a[1] for a in arcs], np.int32)


def decompose(ctx, copies, arcs, iterations, aggressive, compact=False):
    src, dst = arc_arrays(arcs)
    with capi.match_decompose_views(ctx, np.array(copies, np.int64), src, dst, iterations, aggressive, compact=compact) as r:
        got = {k: getattr(r, k).copy() for k in FIELDS}
        if compact:
            got["bare"], got["n_bare"] = r.bare.copy(), r.n_bare
    return got


def assert_fields(got, comps, what):
    for k, want in zip(FIELDS, mc.arrays(comps)):
        assert got[k].dtype == want.dtype and np.array_equal(got[k], want), (what, k)


# ---- raw fields -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [1, 2, 4, 10])
@pytest.mark.parametrize("name", [f for f in mc.FAMILIES if f != "staircases"])
def test_every_field_of_every_component_equals_the_model(ctx, name, iterations):
    copies, _ = family(name)
    for aggressive in (False, True):
        got = decompose(ctx, copies, ranked(name), iterations, aggressive)
        assert_fields(got, expected(name, iterations, aggressive), (name, iterations, aggressive))
        how = capi.match_last_run(ctx)
        assert how["key_mode"] == capi.MATCH_KEYS_POSITION
        rerun = mc.unsettled(expected_and_needed(name, iterations, aggressive)[1])
        assert how["checked_rerun"] == rerun
        if not aggressive:                                         # (the extra round starts from every segment again, with 4 iterations)
            assert rerun == (name == "zigzags")                    # the 40-arc zig-zag takes 20 arcs one iteration after the other


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_the_library_ranks_the_arcs_as_the_model_does(name):
    copies, juncs = family(name)
    e = np.zeros(len(juncs), capi.EDGE_DTYPE)
    u, v, w = (np.array(x, np.int64) for x in zip(*juncs)) if juncs else (np.zeros(0, np.int64),) * 3
    e["left"], e["oL"], e["right"], e["oR"] = u >> 1, u & 1, v >> 1, v & 1
    e["counts"][:, 0], e["counts"][:, 3] = w // 2, w - w // 2
    cp, src, dst, weight = capi.match_arcs_from_edges(np.array(copies, np.int32), e, min_count=0)
    assert list(zip(src.tolist(), dst.tolist(), weight.tolist())) == ranked(name) and cp.tolist() == list(copies)


@pytest.mark.parametrize("k", mc.ZIGZAG_ARCS)
def test_zigzags_around_the_enqueued_iteration_counts(ctx, k):
    """k arcs of which ceil(k / 2) are taken, one per matching iteration: 7 iterations are enqueued for the first round, so from
    k = 15 on (8 needed) the round has not settled and the host-checked run, in batches of 16, produces the result"""
    copies, juncs = mc.zigzag(k)
    arcs = mc.rank_arcs(juncs)
    for aggressive in (False, True):
        needed = []
        want = mc.components(len(copies), copies, arcs, 4, aggressive, needed)
        assert needed[0] == (0, (k + 1) // 2) and (not aggressive or needed[-1] == (4, (k + 1) // 2))
        got = decompose(ctx, copies, arcs, 4, aggressive)
        assert_fields(got, want, (k, aggressive))
        how = capi.match_last_run(ctx)
        assert how["checked_rerun"] == mc.unsettled(needed) == ((k + 1) // 2 >= (4 if aggressive else 7))
        assert how["key_mode"] == capi.MATCH_KEYS_POSITION
        if how["checked_rerun"]:
            assert how["rounds"] == 4 + aggressive and how["iterations"] >= (k + 1) // 2 and how["iterations"] % 16 == 0


@pytest.mark.parametrize("iterations", mc.STAIRCASE_ITERATIONS)
@pytest.mark.parametrize("k", mc.STAIRCASE_LENGTHS)
def test_staircases_through_the_round_groups(ctx, k, iterations):
    """one segment dies per round: the graph is alive for exactly k rounds, around the groups of rounds the host enqueues between
    looks at the state; with `aggressive` the extra round is numbered `iterations` however early the graph died"""
    copies, juncs = mc.staircase(k)
    arcs = mc.rank_arcs(juncs)
    for aggressive in (False, True):
        want = mc.components(k, copies, arcs, iterations, aggressive)
        got = decompose(ctx, copies, arcs, iterations, aggressive)
        assert_fields(got, want, (k, iterations, aggressive))
        if aggressive:
            assert got["iter"][-1] == iterations and got["verts"][got["off"][-2]:].tolist() == [2 * s for s in range(k)]
        how = capi.match_last_run(ctx)
        assert not how["checked_rerun"]                            # (every arc of the path is the best of both its slots at once)
        assert min(k, iterations) + aggressive <= how["rounds"] <= iterations + aggressive
        if (k, iterations, aggressive) == (12, 12, False):
            assert how["rounds"] == 12
        if (k, iterations) == (4, 12):
            assert how["rounds"] < 12                              # nobody keeps a copy after round 3: the host stops (or jumps to the extra round)


def test_union_of_all_staircases(ctx):
    copies, _ = family("staircases")
    for iterations in mc.STAIRCASE_ITERATIONS:
        for aggressive in (False, True):
            assert_fields(decompose(ctx, copies, ranked("staircases"), iterations, aggressive), expected("staircases", iterations, aggressive),
                          (iterations, aggressive))


@pytest.mark.parametrize("name", list(mc.FAMILIES))
def test_compact_form_equals_the_model(ctx, name):
    copies, _ = family(name)
    for aggressive in (False, True):
        listed, bare, n_bare = mc.compact(expected(name, 4, aggressive), len(copies), ranked(name))
        got = decompose(ctx, copies, ranked(name), 4, aggressive, compact=True)
        assert_fields(got, listed, (name, aggressive))
        assert np.array_equal(got["bare"], bare) and got["n_bare"] == n_bare


@pytest.mark.parametrize("which", range(12))
def test_bare_segments_at_the_word_boundary(ctx, which):
    """63, 64 and 65 segments, alone in the call: bare segments before, between and behind the arc-bearing ones, full and compact"""
    copies, juncs = mc.bare_graphs()[which]
    arcs = mc.rank_arcs(juncs)
    for aggressive in (False, True):
        comps = mc.components(len(copies), copies, arcs, 2, aggressive)
        assert_fields(decompose(ctx, copies, arcs, 2, aggressive), comps, (which, aggressive))
        listed, bare, n_bare = mc.compact(comps, len(copies), arcs)
        got = decompose(ctx, copies, arcs, 2, aggressive, compact=True)
        assert_fields(got, listed, (which, aggressive))
        assert np.array_equal(got["bare"], bare) and got["n_bare"] == n_bare and len(got["bare"]) == (len(copies) + 63) // 64


# ---- knobs ------------------------------------------------------------------------------------------------------------------------
def test_every_setting_of_the_knobs_gives_the_same_bytes(ctx):
    copies, _ = family("all")
    base = decompose(ctx, copies, ranked("all"), 10, True)
    assert_fields(base, expected("all", 10, True), "defaults")
    try:
        for option, values in (("iters_per_round", (0, 1, 2, 7, 64)), ("decomp_grid", (1, 3, 256, 0, 65536))):
            for value in values:
                ctx.match_set_option(option, value)
                got = decompose(ctx, copies, ranked("all"), 10, True)
                for k in FIELDS:
                    assert got[k].tobytes() == base[k].tobytes(), (option, value, k)
                if option == "iters_per_round" and value == 1:
                    assert capi.match_last_run(ctx)["checked_rerun"]
            ctx.match_set_option(option, 0)
    finally:
        ctx.match_set_option("iters_per_round", 0)
        ctx.match_set_option("decomp_grid", 0)


# ---- degenerate inputs --------------------------------------------------------------------------------------------------------------
def test_degenerate_graphs(ctx):
    for aggressive in (False, True):
        got = decompose(ctx, [], [], 3, aggressive)
        assert_fields(got, [], "no segment")
        assert capi.match_last_run(ctx) == dict(key_mode=0, checked_rerun=False, rounds=0, iterations=0)
        copies = [2, 1, 3, 1, 1]
        assert_fields(decompose(ctx, copies, [], 3, aggressive), mc.components(5, copies, [], 3, aggressive), "no arc")
        loop = mc.rank_arcs([(0, 0, 5)])
        assert loop == [(0, 0, 5), (1, 1, 5)]
        for c in (1, 3):
            want = mc.components(1, [c], loop, 3, aggressive)
            assert want[0] == (mc.CYCLE, 0, 0, [0])
            assert_fields(decompose(ctx, [c], loop, 3, aggressive), want, ("self loop", c))


def test_bad_arguments_are_refused_on_the_host(ctx):
    copies, arcs = [1, 1], mc.rank_arcs([(0, 2, 5)])
    decompose(ctx, copies, arcs, 1, False)
    before = capi.match_last_run(ctx)
    with pytest.raises(capi.PalaceError):
        decompose(ctx, copies, arcs, 0, False)                     # iterations = 0
    with pytest.raises(capi.PalaceError, match="arc endpoint out of range"):
        decompose(ctx, copies, [(0, 4, 5), (5, 1, 5)], 1, False)   # 4 = 2 * n_segs
    with pytest.raises(capi.PalaceError, match="arc endpoint out of range"):
        decompose(ctx, copies, [(-1, 2, 5)], 1, False)
    assert capi.match_last_run(ctx) == before                      # nothing ran
    assert_fields(decompose(ctx, copies, arcs, 1, False), mc.components(2, copies, arcs, 1), "the context still works")


# ---- palace_match_greedy ------------------------------------------------------------------------------------------------------------
def sequential_greedy(n, src, dst, alive):
    nxt, prv, arc = [-1] * n, [-1] * n, [-1] * n
    for e, (u, v) in enumerate(zip(src, dst)):                     # arc id = rank
        if alive[u] and alive[v] and nxt[u] < 0 and prv[v] < 0:
            nxt[u], prv[v], arc[u] = v, u, e
    return nxt, prv, arc


def greedy_case(which):
    rng = np.random.Generator(np.random.PCG64(31))
    if which == "hub":                                             # 2 000 out-arcs of vertex 0; the heads of all but the last are dead or taken by a better arc
        n, heads = 4000, np.arange(1, 2001)
        alive = np.ones(n, np.uint8)
        alive[heads[:-1:2]] = 0
        takers = np.arange(2001, 4000)
        src = np.concatenate([takers, np.zeros(2000, np.int64)])
        dst = np.concatenate([heads[:-1], heads])
        return n, src, dst, alive
    if which == "chain":                                           # arc e shares a slot with arc e + 1: 20 of the 40 are taken, one per round
        copies, juncs = mc.zigzag(40)
        src, dst = [j[0] for j in juncs], [j[1] for j in juncs]
        return 2 * len(copies), np.array(src), np.array(dst), np.ones(2 * len(copies), np.uint8)
    n = int(which)
    m = 0 if n == 0 else 3 * n
    src, dst = (rng.integers(0, n, m), rng.integers(0, n, m)) if n else (np.zeros(0, np.int64),) * 2      # any digraph: loops, parallel arcs, no conjugates
    return n, src, dst, (rng.random(n) < 0.8).astype(np.uint8)


@pytest.mark.parametrize("which", ["0", "1", "255", "256", "257", "1000", "hub", "chain"])
def test_greedy_matching_equals_the_sequential_greedy(ctx, which):
    n, src, dst, alive = greedy_case(which)
    want = sequential_greedy(n, src.tolist(), dst.tolist(), alive.tolist())
    nxt, prv, arc, rounds = capi.match_greedy(ctx, n, src, dst, alive)
    assert (nxt.tolist(), prv.tolist(), arc.tolist()) == want
    assert rounds % 4 == 0
    if which == "hub":
        assert want[0][0] == 2000 and alive[1:2000:2].sum() == 0
    if which == "chain":
        assert sum(e >= 0 for e in want[2]) == 20 and rounds >= 20
    if which == "1000":
        assert sum(e >= 0 for e in want[2]) > 100 and (alive == 0).sum() > 100


# ---- palace_stage04_match: one-word and two-word keys --------------------------------------------------------------------------------
def stage04(ctx, copies, juncs, lines, iterations, aggressive, use_paths):
    """every contig a seed, min_count 0: the filtered graph is the graph (checked from counts()); -> the compact result's arrays, the
    counts and palace_match_last_run"""
    n = len(copies)
    names = ["EDGE_%07d_length_500_cov_3.0" % (i + 1) for i in range(n)]               # (name order = index order: filtered segment = contig)
    off = np.zeros(len(lines) + 1, np.int64)
    np.cumsum([len(l) for l in lines], out=off[1:])
    tok = np.array([t for l in lines for t in l], np.int32)
    e = np.zeros(len(juncs), capi.EDGE_DTYPE)
    u, v, w = (np.array(x, np.int64) for x in zip(*juncs))
    e["left"], e["oL"], e["right"], e["oR"] = u >> 1, u & 1, v >> 1, v & 1
    e["counts"][:, 0], e["counts"][:, 1], e["counts"][:, 3] = w // 2, w % 2, w // 2                  # the weight is the sum of the counters
    st = capi.Stage04(ctx, np.ones(n, np.uint8), np.full(n, 500, np.int32), stage04_io.name_ranks(names), stage04_io.name_lengths(names), off, tok,
                      min_count=0)
    bufs = [ctx.upload(e.view(np.uint8).reshape(-1)), ctx.upload(np.array([len(e)], np.int64)), ctx.upload(np.array(copies, np.int32))]
    try:
        st.filter(bufs[0].ptr, bufs[1].ptr, len(e))
        st.match(bufs[0].ptr, bufs[2].ptr, iterations, aggressive, use_paths)
        res, contig_of = st.result()
        got = {k: getattr(res, k).copy() for k in FIELDS}
        got["bare"], got["n_bare"] = res.bare.copy(), res.n_bare
        assert np.array_equal(contig_of, np.arange(n))
        counts = st.counts()
        assert counts["juncs"] == counts["kept_pass2"] == len(e) and counts["kept_pass3_more"] == 0 and counts["segs_filtered"] == n
        return got, counts, capi.match_last_run(ctx)
    finally:
        st.close()
        for b in bufs:
            b.free()


def assert_stage04(got, counts, copies, arcs, comps, what):
    listed, bare, n_bare = mc.compact(comps, len(copies), arcs)
    assert counts["arcs"] == len(arcs)
    assert_fields(got, listed, what)
    assert np.array_equal(got["bare"], bare) and got["n_bare"] == n_bare


@functools.lru_cache(maxsize=None)
def keys_case(name, aggressive):
    copies, juncs, lines = mc.backed_case() if name == "paths" else family(name) + ([],)
    arcs, needed = mc.rank_arcs(juncs, mc.backed_arcs(lines)), []
    return copies, juncs, lines, arcs, mc.components(len(copies), copies, arcs, 10, aggressive, needed), needed


@pytest.mark.parametrize("iters_per_round", [0, 1])
@pytest.mark.parametrize("one_word_keys", [1, 0])
@pytest.mark.parametrize("name", ["settling", "paths", "all"])
def test_stage04_in_both_key_modes_equals_the_model(ctx, name, one_word_keys, iters_per_round):
    """the union of the families without paths, and small graphs with contigs.paths lines over them (a path-backed arc ranks before
    an unbacked one of equal weight); by one-word keys, by two-word keys as enqueued (klo halves by iteration parity and their
    resets), and both through the host-checked run.  "all" holds the long zig-zags: its rounds never settle as enqueued."""
    try:
        ctx.match_set_option("one_word_keys", one_word_keys)
        ctx.match_set_option("iters_per_round", iters_per_round)
        for aggressive in (False, True):
            copies, juncs, lines, arcs, comps, needed = keys_case(name, aggressive)
            got, counts, how = stage04(ctx, copies, juncs, lines, 10, aggressive, use_paths=bool(lines))
            assert_stage04(got, counts, copies, arcs, comps, (name, one_word_keys, iters_per_round, aggressive))
            rerun = mc.unsettled(needed, 1, 1) if iters_per_round else mc.unsettled(needed)
            if not aggressive:                                     # the premise of this test: which runs go through as enqueued
                assert rerun == (iters_per_round == 1 or name == "all")
            assert how["checked_rerun"] == rerun
            assert how["key_mode"] == (capi.MATCH_KEYS_ONE_WORD if one_word_keys and not rerun else capi.MATCH_KEYS_TWO_WORDS)
    finally:
        ctx.match_set_option("one_word_keys", 1)
        ctx.match_set_option("iters_per_round", 0)


@pytest.mark.parametrize("over", [0, 1])
def test_stage04_at_the_weight_edge_of_the_one_word_key(ctx, over):
    """The one-word key holds [weight term | not backed | class of (u, v)] with vbits = bits of the largest sub-graph vertex id for
    each end and what is left of 51 bits (at most 40) for the weight (st4_sub_kernel): the heaviest junction at exactly the largest
    weight that fits stays one-word, one more falls back to two words.  Fifteen junctions tie at that weight, twelve of them a
    zig-zag in which only the class -- klo in the two-word form -- says which arc a slot takes, six iterations long."""
    small = mc.three_segment_graphs()[:190]
    tie = ([1] * 13, [(2 * (j // 2 + (j & 1)), 2 * (7 + j // 2), 0) for j in range(12)])              # a0 -> b0 <- a1 -> b1 ..: equal weights
    hub = ([1] * 4, [(0, 2, 0), (0, 4, 0), (0, 7, 0)])
    copies, juncs = mc.union([tie, hub] + small)
    n_sub = len(copies) - len(mc.bare_segments(len(copies), juncs))
    vbits = max(1, 2 * n_sub - 1).bit_length()
    wbits = min(40, 51 - 2 * vbits)
    wmax = (1 << wbits) - 1
    assert (vbits, wbits) == (11, 29) and wmax < 1 << 32                                              # (a junction's counters are 32-bit)
    juncs = [(u, v, w or wmax + over) for u, v, w in juncs]
    assert sum(w == wmax + over for _, _, w in juncs) == 15 and max(w for _, _, w in juncs) == wmax + over
    arcs = mc.rank_arcs(juncs)
    for aggressive in (False, True):
        needed = []
        comps = mc.components(len(copies), copies, arcs, 10, aggressive, needed)
        assert needed[0] == (0, 6) and mc.unsettled(needed) == aggressive      # (the extra round has 4 iterations for the zig-zag's 6)
        got, counts, how = stage04(ctx, copies, juncs, [], 10, aggressive, use_paths=False)
        assert_stage04(got, counts, copies, arcs, comps, (over, aggressive))
        assert how["checked_rerun"] == aggressive
        assert how["key_mode"] == (capi.MATCH_KEYS_TWO_WORDS if over or aggressive else capi.MATCH_KEYS_ONE_WORD)
