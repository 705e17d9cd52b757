"""The path / cycle decomposition as an exact model, and the small graphs it is held against (no tests in here).

The model is a third statement of DESIGN.md section 7, written from that prose and from what include/palace_hip.h documents
for palace_match_decompose -- not from csrc/decomp.hip and not from oracle/match_oracle.cpp.  Unlike tests/match_bruteforce.py
and the oracle it does not format: `components` returns every component with every documented field (kind, iter, open_at,
vertices) in emission order, repeats and later-round singletons included, so that the arrays a device call hands back can be
compared element for element.  tests/test_host_match_model.py makes the three statements agree on every family below
before tests/test_gpu_match_abi.py lets any of them judge the device.

Vertices are oriented segments, 2 * segment + (orientation == '-'); the conjugate of the arc (u, v) is (v ^ 1, u ^ 1).
A graph is (copies, juncs): copy number per segment, junctions as oriented (u, v, weight) triples.

    python -m tests.match_cases        # per family: graphs, paths, cycles, components that are their own conjugate
"""
import numpy as np

PATH, CYCLE = 0, 1


def conj(a):
    return (a[1] ^ 1, a[0] ^ 1)


def rank_arcs(juncs, backed=()):
    """Junctions (u, v, w) -> the arcs [(u, v, w)] in rank order: every junction and its conjugate (an arc that is its own
    conjugate once), equal arcs merged with their weights added; weight descending, class min(arc, conjugate) ascending,
    (u, v) ascending -- the rule of palace_match_arcs_from_edges.  `backed`: arcs (u, v) that a contigs.paths line backs
    (matching -l, palace_stage04_match with use_paths): they and their conjugates exist with weight 0 if no junction names
    them, and rank before unbacked arcs of equal weight."""
    weight, is_backed = {}, set()
    for u, v, w in juncs:
        for a in {(u, v), conj((u, v))}:
            weight[a] = weight.get(a, 0) + w
    for a in backed:
        for x in {tuple(a), conj(a)}:
            weight.setdefault(x, 0)
            is_backed.add(x)
    order = sorted(weight, key=lambda a: (-weight[a], a not in is_backed, min(a, conj(a)), a))
    return [(u, v, weight[(u, v)]) for u, v in order]


def dominant_iterations(arcs, alive):
    """How many matching iterations of the device's kind a round takes: in each, every arc that is the best
    remaining one of both its tail's out slot and its head's in slot is taken.  The result is the sequential greedy matching
    however many it takes; the number only says whether the iterations a round was given sufficed -- a round that still took
    an arc in the last one it was given has not settled and the host-checked run takes over."""
    open_out, open_in, rest, n = set(alive), set(alive), list(enumerate(arcs)), 0
    while True:
        rest = [(i, a) for i, a in rest if a[0] in open_out and a[1] in open_in]
        best_out, best_in = {}, {}
        for i, (u, v) in rest:
            best_out.setdefault(u, i); best_in.setdefault(v, i)
        taken = [a for i, a in rest if best_out[a[0]] == i and best_in[a[1]] == i]
        if not taken:
            return n
        n += 1
        for u, v in taken:
            open_out.discard(u); open_in.discard(v)


def components(n_segs, copies, ranked, iterations, aggressive=False, needed=None):
    """-> [(kind, iter, open_at, verts)] in emission order, as include/palace_hip.h documents the result of
    palace_match_decompose; nothing is filtered.  needed: a list that gets (round, dominant_iterations) of every round with a
    live segment."""
    arcs = [(a[0], a[1]) for a in ranked]
    rank_of = {a: i for i, a in enumerate(arcs)}
    left = [max(1, int(c)) for c in copies]
    rounds = iterations + (1 if aggressive else 0)
    out = []
    for t in range(rounds):
        if aggressive and t == rounds - 1:
            left = [1] * n_segs                                    # the copy-number blind round
        live = [v for v in range(2 * n_segs) if left[v >> 1] > 0]
        if not live:
            continue
        alive = set(live)
        if needed is not None:
            needed.append((t, dominant_iterations(arcs, alive)))
        succ, pred = {}, {}
        for u, v in arcs:                                          # sequential greedy in rank order
            if u in alive and v in alive and u not in succ and v not in pred:
                succ[u], pred[v] = v, u
        found, on_path = [], set()
        for v in live:                                             # open walks start where nothing leads in
            if v in pred:
                continue
            walk = [v]
            while walk[-1] in succ:
                walk.append(succ[walk[-1]])
            on_path.update(walk)
            if walk[0] <= walk[-1] ^ 1:                            # the conjugate path starts at the flipped last vertex
                found.append((PATH, walk))
        seen = set()
        for v in live:                                             # what is left lies on closed walks; ascending: v is its cycle's smallest
            if v in on_path or v in seen:
                continue
            walk = [v]
            while succ[walk[-1]] != v:
                walk.append(succ[walk[-1]])
            seen.update(walk)
            if walk[0] <= min(x ^ 1 for x in walk):                # the conjugate cycle, rotated to ITS smallest vertex
                found.append((CYCLE, walk))
        found.sort(key=lambda c: c[1][0])
        for kind, vs in found:
            times = {}
            for x in vs:
                times[x >> 1] = times.get(x >> 1, 0) + 1
            pay = max(1, min(left[s] // k for s, k in times.items()))
            for s, k in times.items():
                left[s] = max(0, left[s] - pay * k)
            open_at = 0
            if kind == CYCLE:
                worst = max(range(len(vs)), key=lambda i: rank_of[(vs[i], vs[(i + 1) % len(vs)])])
                open_at = (worst + 1) % len(vs)
            out.append((kind, t, open_at, vs))
    return out


def model(graph, iterations, aggressive=False, backed=()):
    copies, juncs = graph
    return components(len(copies), copies, rank_arcs(juncs, backed), iterations, aggressive)


def arrays(comps):
    """the components as the five arrays of a palace_match_result: off, verts, kind, iter, open_at"""
    off = np.zeros(len(comps) + 1, np.int64)
    np.cumsum([len(c[3]) for c in comps], out=off[1:])
    verts = np.array([v for c in comps for v in c[3]], np.int32)
    return (off, verts, np.array([c[0] for c in comps], np.uint8), np.array([c[1] for c in comps], np.int32),
            np.array([c[2] for c in comps], np.int32))


def bare_segments(n_segs, arcs):
    """segments no arc (u, v, ..) touches: what a compact result gives as bits instead of listing them"""
    touched = {x >> 1 for a in arcs for x in a[:2]}
    return [s for s in range(n_segs) if s not in touched]


def compact(comps, n_segs, arcs):
    """(the components a compact result lists, the bare bit set as uint64 words, n_bare)"""
    bare = set(bare_segments(n_segs, arcs))
    words = np.zeros((n_segs + 63) // 64, np.uint64)
    for s in bare:
        words[s >> 6] |= np.uint64(1) << np.uint64(s & 63)
    return [c for c in comps if (c[3][0] >> 1) not in bare], words, len(bare)


def is_self_conjugate(kind, vs):
    twin = [x ^ 1 for x in reversed(vs)]
    if kind == CYCLE:
        k = twin.index(min(twin))
        twin = twin[k:] + twin[:k]
    return twin == list(vs)


def text(comps, names, self_loops=False, break_cycles=False):
    """(linear text, cycle text) by the executable's rules: a path line once, a one-vertex path only in round 0; a cycle once,
    as `iter <round>` + line, one-vertex cycles as `self` + line behind the others under -s; under -b every listed cycle also
    as a path opened at open_at."""
    tok = lambda v: names[v >> 1] + "+-"[v & 1]
    line = lambda vs: "\t".join(tok(v) for v in vs) + "\n"
    lin, cyc, selfs, seen_l, seen_c = [], [], [], set(), set()
    for kind, t, open_at, vs in comps:
        body = line(vs)
        if kind == PATH:
            if (len(vs) > 1 or t == 0) and body not in seen_l:
                seen_l.add(body); lin.append(body)
            continue
        if body in seen_c:
            continue
        seen_c.add(body)
        if len(vs) == 1 and self_loops:
            selfs.append("self\n" + body)
        else:
            cyc.append("iter %d\n" % t + body)
        if break_cycles:
            opened = line(vs[open_at:] + vs[:open_at])
            if opened not in seen_l:
                seen_l.add(opened); lin.append(opened)
    return "".join(lin), "".join(cyc + selfs)


def names_for(n_segs):
    return ["EDGE_%d_length_%d_cov_2.0" % (i + 1, 100 + i) for i in range(n_segs)]


def junc_records(juncs):
    """(u, v, w) -> (left, '+'|'-', right, '+'|'-', w), the form tests/match_bruteforce.py and the SEG/JUNC text take"""
    return [(u >> 1, "+-"[u & 1], v >> 1, "+-"[v & 1], w) for u, v, w in juncs]


def union(graphs):
    """many graphs as one: segment ids shifted so that the graphs are disjoint"""
    copies, juncs = [], []
    for cp, js in graphs:
        base = 2 * len(copies)
        copies += list(cp)
        juncs += [(base + u, base + v, w) for u, v, w in js]
    return copies, juncs


# ---- the case families: each returns the list of its graphs; FAMILIES maps a name to (copies, juncs) of their union ------------
def arc_classes(n_segs):
    """one arc per conjugate class of the arcs on n_segs segments (the smaller of arc and conjugate)"""
    V = 2 * n_segs
    return sorted({min((u, v), conj((u, v))) for u in range(V) for v in range(V)})


def _weightings(rng, n):
    return [[7] * n, [int(x) for x in rng.choice([5, 6, 9], n)], [int(x) for x in rng.choice([5, 6, 9], n)]]


def two_segment_graphs():
    """every subset of the 10 arc classes on two segments x 3 weightings x 3 copy-number pairs: 9 216 graphs"""
    cls = arc_classes(2)
    assert len(cls) == 10 and sum(a == conj(a) for a in cls) == 4 and sum(a[0] == a[1] for a in cls) == 2
    rng = np.random.Generator(np.random.PCG64(2))
    out = []
    for mask in range(1 << len(cls)):
        chosen = [a for i, a in enumerate(cls) if mask >> i & 1]
        for ws in _weightings(rng, len(chosen)):
            for cp in ((1, 1), (2, 3), (4, 1)):
                out.append((list(cp), [(u, v, w) for (u, v), w in zip(chosen, ws)]))
    return out


def three_segment_graphs(n_subsets=3334):
    """seeded subsets of the 21 arc classes on three segments x 3 weightings, copies drawn from 1..4: about 10 000 graphs"""
    cls = arc_classes(3)
    assert len(cls) == 21
    rng = np.random.Generator(np.random.PCG64(3))
    out = []
    for _ in range(n_subsets):
        p = rng.choice([0.15, 0.3, 0.5])
        chosen = [a for a in cls if rng.random() < p]
        for ws in _weightings(rng, len(chosen)):
            out.append(([int(c) for c in rng.integers(1, 5, 3)], [(u, v, w) for (u, v), w in zip(chosen, ws)]))
    return out


def ring(verts, weights):
    return [(verts[i], verts[(i + 1) % len(verts)], weights[i]) for i in range(len(verts))]


def ring_graphs():
    out = []
    for n in range(1, 10):                                         # s0+ -> s1+ -> .. -> s0+, the weakest arc at every position
        fwd = [2 * s for s in range(n)]
        for weak in list(range(n)) + [None]:                       # None: all weights equal, the rank alone names the worst arc
            out.append(([1 + (s + n) % 3 for s in range(n)], ring(fwd, [5 if i == weak else 9 for i in range(n)])))
    # the ring that is its own conjugate: x1 .. xk xk' .. x1' -- every segment lies on it twice
    for k, copies in [(4, [1, 2, 3, 5]), (4, [5, 3, 2, 1])] + [(k, [c] * k) for k in (1, 2, 3) for c in (1, 2, 3, 5)]:
        half = [2 * s + (s & 1) for s in range(k)]
        vs = half + [x ^ 1 for x in reversed(half)]
        for weak in (None, 0, k - 1, k):
            out.append((copies, ring(vs, [5 if i == weak else 9 for i in range(len(vs))])))
    # two rings through segment 0, which has two copies
    for wa, wb in ((9, 6), (6, 9), (7, 7)):
        for others in (1, 2):
            a, b = ring([0, 2, 4], [wa] * 3), ring([0, 6, 8], [wb] * 3)
            out.append(([2] + [others] * 4, a + b))
    out.append(([2, 1, 1, 3, 3], ring([0, 2, 4], [9, 5, 9]) + ring([0, 7, 9], [8, 8, 6])))
    return out


def hairpin_graphs():
    out = []
    for c in (1, 2, 3):
        out.append(([c], [(0, 1, 9)]))                             # a+ -> a-
        out.append(([c], [(1, 0, 9)]))                             # a- -> a+
        for cx in (1, 2, 3):                                       # x+ -> a+ -> a- -> x-
            out.append(([cx, c], [(0, 2, 9), (2, 3, 8)]))
            out.append(([c, cx], [(2, 0, 6), (0, 1, 9)]))
            out.append(([cx, c, 2], [(4, 0, 7), (0, 2, 9), (2, 3, 8)]))     # y+ -> x+ -> a+ -> a- -> x- -> y-
    return out


ZIGZAG_ARCS = (1, 6, 7, 8, 15, 16, 17, 31, 32, 33, 40)


def zigzag(k):
    """k arcs of ascending weight, consecutive ones sharing a slot: a0 -> b0 <- a1 -> b1 <- a2 ..; the greedy matching takes
    every second one from the heavy end, and a device iteration can take only one of them"""
    n_a = (k - 1) // 2 + ((k - 1) & 1) + 1
    juncs = [(2 * (j // 2 + (j & 1)), 2 * (n_a + j // 2), 5 + j) for j in range(k)]
    n = 1 + max(max(u, v) >> 1 for u, v, _ in juncs)
    return [1 + (s % 3) for s in range(n)], juncs


def zigzag_graphs():
    return [zigzag(k) for k in ZIGZAG_ARCS]


STAIRCASE_LENGTHS = (4, 5, 6, 10, 11, 12)
STAIRCASE_ITERATIONS = (1, 5, 6, 10, 12)


def staircase(k):
    """the path s1 .. sk with copies 1 .. k: every round pays one copy and loses the first segment, k rounds"""
    return list(range(1, k + 1)), [(2 * s, 2 * s + 2, 9) for s in range(k - 1)]


def staircase_graphs():
    return [staircase(k) for k in STAIRCASE_LENGTHS]


def bare_graphs():
    out = []
    for n in (63, 64, 65):
        cp = [1 + (s % 4) for s in range(n)]
        out.append((cp, [(2 * 0, 2 * (n - 1), 9), (2 * 31 + 1, 2 * 32, 7)]))                 # arcs on segment 0 and the last, bare between
        out.append((cp, [(2 * 1, 2 * (n - 2) + 1, 9), (2 * 30, 2 * 30, 6)]))                 # segment 0 and the last bare
        out.append((cp, [(2 * s, 2 * s + 4, 9) for s in range(0, n - 2, 4)]))                # every other pair
        out.append((cp, []))                                                                 # nothing but bare segments
    return out


def backed_case(n_graphs=300, seed=11):
    """small random graphs with contigs.paths lines over them -> (copies, juncs, lines), a line = the oriented vertices it names;
    consecutive ones are path-backed arcs (matching -l)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    graphs, lines, base = [], [], 0
    for _ in range(n_graphs):
        n = int(rng.integers(2, 6))
        juncs = {}
        for _ in range(int(rng.integers(1, 9))):
            a = (int(rng.integers(0, 2 * n)), int(rng.integers(0, 2 * n)))
            juncs[min(a, conj(a))] = int(rng.choice([5, 5, 6, 9]))                 # (one junction per class, as generateGraph aggregates)
        graphs.append(([int(c) for c in rng.integers(1, 4, n)], [(u, v, w) for (u, v), w in juncs.items()]))
        for _ in range(int(rng.integers(0, 3))):
            lines.append([base + int(rng.integers(0, 2 * n)) for _ in range(int(rng.integers(1, 5)))])
        base += 2 * n
    copies, juncs = union(graphs)
    return copies, juncs, lines


def backed_arcs(lines):
    return [a for toks in lines for a in zip(toks, toks[1:])]


FAMILY_GRAPHS = dict(two_segment=two_segment_graphs, three_segment=three_segment_graphs, rings=ring_graphs, hairpins=hairpin_graphs,
                     zigzags=zigzag_graphs, staircases=staircase_graphs, bare=bare_graphs)
FAMILIES = {name: (lambda f=f: union(f())) for name, f in FAMILY_GRAPHS.items()}
# what each family exists for: it must produce some of each
NEEDS = dict(two_segment=("paths", "cycles", "self_conjugate"), three_segment=("paths", "cycles", "self_conjugate"),
             rings=("cycles", "self_conjugate"), hairpins=("paths", "self_conjugate"), zigzags=("paths",), staircases=("paths",),
             bare=("paths",))


def unsettled(needed, first=7, later=4):
    """whether a decomposition whose rounds need these iterations is redone with the host checking: include/palace_hip.h gives the
    first round 7 enqueued iterations and every later one 4 ("iters_per_round" n: both n)"""
    return any(n >= (first if t == 0 else later) for t, n in needed)


def census(name, iterations=4):
    graphs = FAMILY_GRAPHS[name]()
    comps = model(union(graphs), iterations)
    return dict(graphs=len(graphs), paths=sum(c[0] == PATH for c in comps), cycles=sum(c[0] == CYCLE for c in comps),
                self_conjugate=sum(is_self_conjugate(c[0], c[3]) for c in comps))


if __name__ == "__main__":
    import sys
    bad = []
    for fam in FAMILY_GRAPHS:
        c = census(fam)
        print("%-14s graphs %6d  paths %6d  cycles %6d  own conjugate %6d" % (fam, c["graphs"], c["paths"], c["cycles"], c["self_conjugate"]))
        bad += ["%s: no %s" % (fam, k) for k in NEEDS[fam] if not c[k]]
    if bad:
        sys.exit("; ".join(bad))
