"""Planted per-channel hit patterns at the edges of the eref window rules (Phase B) -- no GPU needed.

Every other eref test makes its hits by sampling reads from the refs: long runs, all three channels at once, sentinels in
proportion.  Here the hits are PLANTED position by position and channel by channel:

  * a 32-base read that equals the ref's 32-mer at j sets all three channels of j (counted three times: a hit needs count 3);
  * the same read with ONE substituted base keeps a subset of the channels -- every channel reads one one-bit projection of
    each base and a substitution preserves exactly one of the three; which subset survives depends on the canonical
    min(fwd, rc), so `plant` searches the (offset, substitute) pairs for the wanted subset.

The planted intent is never the expectation (32-bit keys collide by chance): the expectation is `rows_model` over
`realized_bits`, the oracle's own table and indices.  A case also carries a CLAIM over the model's intermediate values (such as
"the largest all-count of any window is exactly three_min") which shows that the input sits on the edge it is named after;
claims are asserted, never filtered -- a case whose claim fails is repaired here (SEED_BUMP).

    python -m tests.scan_cases        # per family: refs, bases, plants, edges, refs reported under (450, 425)
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Callable, NamedTuple

import numpy as np

from oracle import binding as orc
from palace_amd import capi, synth

WINDOW = 500
ALL = (0, 1, 2)
GRID = [(0, 0), (1, 0), (0, 1), (1, 1), (500, 500), (501, 0), (0, 501), (100, 250), (250, 100), (450, 425), (425, 376),
        (425, 377)]
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 499, 500, 501, 530, 531, 532, 563, 564, 565, 1023, 1024, 1025, 2047,
           2048, 2049, 4095, 4096, 4097]
# a case's seed is crc32(name) + SEED_BUMP.get(name, 0): bumped where a chance hit (a key collision with another case's reads)
# broke the case's claim
SEED_BUMP: dict = {'no_c0/250_100_c12_short': 1, 'no_c0/450_425_c0_short': 1}


@functools.lru_cache(maxsize=None)
def coder():
    """-> (400-byte index header, choose_coder[96]) of the catalogue: one fixed random coder"""
    hdr = orc.header_from_picks(synth.rng_for(20261).integers(0, 6, size=32))
    return hdr, orc.header_to_cc(hdr)


def ratio_for(T: int) -> float:
    """the ratio that orc.scan_ref (which takes ratios, as the reference does) turns into the INT threshold T"""
    r = (T + 0.5) / WINDOW
    assert capi.window_minimums(r, r) == (T, T), T
    return r


def plant(ref: np.ndarray, j: int, channels, cc=None) -> np.ndarray:
    """A 32-base read whose keys equal exactly the `channels` subset of the ref's three keys at j (raises if there is none)."""
    cc = coder()[1] if cc is None else cc
    want = set(channels)
    assert want and want <= set(ALL) and 0 <= j <= len(ref) - 32
    base = np.array(ref[j:j + 32], dtype=np.uint8)
    keys = orc.index_ref(base, cc)
    if (keys == 0).any():
        raise ValueError(f"position {j}: no valid key in every channel")
    if want == set(ALL):
        return base
    for off in range(32):
        for sub in b"ACGT":
            if sub == (base[off] & 0xDF):
                continue
            r = base.copy()
            r[off] = sub
            k = orc.index_ref(r, cc)
            if {i for i in ALL if k[i] == keys[i]} == want and not (set(k.tolist()) & {int(keys[i]) for i in ALL if i not in want}):
                return r
    raise ValueError(f"position {j}: no single substitution leaves exactly channels {sorted(want)}")


def plant_reads(ref: np.ndarray, j: int, channels, cc=None) -> list:
    """`plant` as a list of reads.  A substitution preserves one projection of its base, so a single read keeps one channel or all
    three; where no single read gives a subset of two, one read per channel does (the channels share the one count table)."""
    try:
        return [plant(ref, j, channels, cc)]
    except ValueError:
        if len(set(channels)) != 2:
            raise
        return [plant(ref, j, (c,), cc) for c in sorted(set(channels))]


def oracle_table(reads, cc) -> orc.CountTable:
    """the oracle's count table with every read counted three times"""
    t = orc.CountTable()
    rs = synth.reads_from_list(list(reads))
    for _ in range(3):
        t.count(rs.bases, rs.offsets, cc)
    return t


def realized_bits(refs, reads, cc, table: orc.CountTable | None = None):
    """per ref the bool array c[0..2][j], j < len - 31: c[i][j] = (idx[3j+i] != 0) & (table[idx[3j+i]] == 3) -- the oracle's bits"""
    t = table or oracle_table(reads, cc)
    out = []
    for s in refs:
        idx = orc.index_ref(s, cc).reshape(-1, 3)
        out.append(((idx != 0) & (t.lookup(idx) == 3)).T.copy() if len(idx) else np.zeros((3, 0), dtype=bool))
    if table is None:
        t.free()
    return out


class Rows(NamedTuple):
    n_intervals: int
    el: int
    good: np.ndarray       # good[j], j < ref_len
    n_edges: int           # rising + falling edges of `good` (a run open at the end closes with one)
    one: np.ndarray        # any-hits among positions (j - 500, j]
    three: np.ndarray      # all-hits among positions (j - 500, j]


def window_counts(bits: np.ndarray, ref_len: int) -> np.ndarray:
    """hits among positions (j - 500, j] for j in [0, ref_len); bits[j] is zero from ref_len - 31 on"""
    cs = np.zeros(ref_len + 1, dtype=np.int64)
    cs[1:1 + len(bits)] = bits
    np.cumsum(cs, out=cs)                                  # cs[k] = hits at positions < k
    j = np.arange(ref_len)
    return cs[j + 1] - cs[np.maximum(0, j - (WINDOW - 1))]


def rows_model(c, ref_len: int, one_min: int, three_min: int, counts=None) -> Rows:
    """slide_window restated with the INT thresholds the C ABI takes; c = the three channels' bits (realized_bits)"""
    if counts is None:
        counts = (window_counts(c[0] | c[1] | c[2], ref_len), window_counts(c[0] & c[1] & c[2], ref_len))
    one, three = counts
    good = (one >= one_min) & (three >= three_min)
    d = np.diff(np.concatenate([[0], good.astype(np.int8), [0]]))
    rising, falling = np.flatnonzero(d == 1), np.flatnonzero(d == -1)     # falling == ref_len: the run was open at the end
    frag = el = prev_end = 0
    for jr, jf in zip(rising.tolist(), falling.tolist()):
        start = max(1, jr - 2 * WINDOW)
        end = min(ref_len, jf + 2 * WINDOW)
        if frag > 0 and start - prev_end < WINDOW:
            el += end - prev_end
        else:
            frag += 1
            el += end - start
        prev_end = end
    return Rows(frag, el, good, len(rising) + len(falling), one, three)


@dataclass
class Case:
    name: str
    family: str
    refs: list                               # np.uint8 arrays
    plants: list                             # (ref of the case, position, channels)
    pairs: list                              # the (one_min, three_min) pairs the case is about
    claim: Callable                          # claim(view): asserts what makes this case the edge it is named after
    first: int = 0                           # catalogue index of refs[0]


class View:
    """what a claim may look at: the model's values for the case's own refs"""

    def __init__(self, cat, case):
        self.cat, self.case = cat, case

    def rows(self, i, T1, T3) -> Rows:
        return self.cat.rows(self.case.first + i, T1, T3)

    def bits(self, i):
        return self.cat.bits[self.case.first + i]

    def length(self, i):
        return len(self.case.refs[i])


def _seed(name):
    return zlib.crc32(name.encode()) + SEED_BUMP.get(name, 0)


def _block(i, a, n, ch=ALL):
    return [(i, a + k, ch) for k in range(n)]


def _edges_of(good):
    d = np.diff(np.concatenate([[0], good.astype(np.int8), [0]]))
    return np.flatnonzero(d == 1), np.flatnonzero(d == -1)


def _tag(ch):
    return "c" + "".join(str(c) for c in ch)


# ---- the families -------------------------------------------------------------------------------------------------------
def family_lengths():
    out = []
    for L in LENGTHS:
        name = f"lengths/{L}"
        ref = synth.random_dna(synth.rng_for(_seed(name)), L)

        def claim(v, L=L):
            assert v.bits(0).shape == (3, max(0, L - 31)) and v.bits(0).all()
            assert bool(v.rows(0, 500, 500).good.any()) == (L >= 531)          # 500 planted positions need 531 bases
            assert v.rows(0, 0, 0)[:2] == ((1, L - 1) if L else (0, 0))
        out.append(Case(name, "lengths", [ref], _block(0, 0, max(0, L - 31)), [], claim))
    return out


def family_exact():
    out = []
    for T1, T3 in ((450, 425), (250, 100), (425, 425)):
        for short in (0, 1):
            name = f"exact/all_{T1}_{T3}" + ("_short" if short else "")
            ref = synth.random_dna(synth.rng_for(_seed(name)), 1500)
            total = min(WINDOW, max(T1, T3) + 40)
            plants = _block(0, 500, T3 - short) + _block(0, 500 + T3, total - T3, (0,))

            def claim(v, T1=T1, T3=T3, short=short):
                r = v.rows(0, T1, T3)
                assert r.three.max() == T3 - short and r.one.max() >= T1 + 30
                assert bool(r.good.any()) == (not short) and (r.el > 0) == (not short)
            out.append(Case(name, "exact", [ref], plants, [(T1, T3)], claim))
        full = min(T3 + 20, T1)
        extras = T1 - full
        for ch in ((0,), (1,), (2,), (1, 2)) if extras else ((0,),):
            for short in (0, 1):
                name = f"exact/any_{T1}_{T3}_{_tag(ch)}" + ("_short" if short else "")
                ref = synth.random_dna(synth.rng_for(_seed(name)), 1500)
                if extras:
                    plants = _block(0, 500, full) + _block(0, 500 + full, extras - short, ch)
                else:
                    plants = _block(0, 500, full - short)

                def claim(v, T1=T1, T3=T3, short=short, full=full, extras=extras):
                    r = v.rows(0, T1, T3)
                    assert r.one.max() == T1 - short and r.three.max() == (full if extras else full - short)
                    assert bool(r.good.any()) == (not short)
                out.append(Case(name, "exact", [ref], plants, [(T1, T3)], claim))
    return out


def _sentinel_case(name, L, a, B, T3, short, from_end):
    ref = synth.random_dna(synth.rng_for(_seed(name)), L)
    sent = [p for p in range(a, a + B) if p % 4 == 0]
    k = T3 - (B - len(sent))                                   # sentinels that must hit for the largest all-count to be T3
    assert 1 <= k <= len(sent)
    chosen = (sent[::-1] if from_end else sent)[:k - short]
    plants = [(0, p, ALL) for p in range(a, a + B) if p % 4] + [(0, p, ALL) for p in chosen]

    def claim(v):
        r = v.rows(0, T3, T3)
        assert r.three.max() == T3 - short and bool(r.good.any()) == (not short)
        allb = v.bits(0).all(axis=0)
        s = np.zeros(L, dtype=bool)
        s[0::4] = True
        hit_sent = window_counts(allb & s[:len(allb)], L)
        if not short:                                          # a passing window with as few sentinel hits as the rule allows
            assert hit_sent[r.good].min() == k and k == max(0, WINDOW // 4 - 1 - (WINDOW - T3)) + 1
    return Case(name, "sentinel", [ref], plants, [(T3, T3), (0, T3)], claim)


def family_sentinel():
    out = []
    for T3 in (376, 377, 378, 400, 425):
        for a in (644, 641, 642, 643, 640, 703):               # block start = 0, 1, 2, 3 mod 4; 0 and 63 mod 64
            for short in (0, 1):
                out.append(_sentinel_case(f"sentinel/T{T3}_a{a}" + ("_short" if short else ""), 1800, a, WINDOW, T3, short,
                                          from_end=bool(a & 1)))
        for short in (0, 1):
            # inside the first 500 positions: the cumulative window [0, 499] decides
            out.append(_sentinel_case(f"sentinel/T{T3}_first" + ("_short" if short else ""), 1200, 0, WINDOW, T3, short, False))
            # the block ends at the ref's last position that has a 32-mer
            out.append(_sentinel_case(f"sentinel/T{T3}_last" + ("_short" if short else ""), 1331, 800, WINDOW, T3, short, True))
    return out


def family_no_c0():
    out = []
    for T1, T3 in ((250, 100), (450, 425)):
        for ch in ((1, 2), (0,)):
            for split in (0, 1):                               # the any-only plants right behind the full ones / 380 positions away
                for short in (0, 1):
                    name = f"no_c0/{T1}_{T3}_{_tag(ch)}" + ("_split" if split else "") + ("_short" if short else "")
                    ref = synth.random_dna(synth.rng_for(_seed(name)), 1700)
                    n_any = T1 - T3 - short
                    a = 600
                    at_any = a if split else a + WINDOW - T1
                    plants = _block(0, a + WINDOW - T3, T3) + _block(0, at_any, n_any, ch)

                    def claim(v, T1=T1, T3=T3, short=short, ch=ch):
                        r = v.rows(0, T1, T3)
                        assert r.three.max() == T3 and r.one.max() == T1 - short and bool(r.good.any()) == (not short)
                        c0 = window_counts(v.bits(0)[0], v.length(0))
                        assert c0.max() == (T3 if ch == (1, 2) else T1 - short)
                    out.append(Case(name, "no_c0", [ref], plants, [(T1, T3)], claim))
    for short in (0, 1):                                       # channel 0 far above three_min, the all-count at it / one short of it
        name = "no_c0/c0_rich" + ("_short" if short else "")
        ref = synth.random_dna(synth.rng_for(_seed(name)), 1700)
        plants = _block(0, 600, 100 - short) + _block(0, 700, 300, (0,))

        def claim(v, short=short):
            r = v.rows(0, 250, 100)
            assert window_counts(v.bits(0)[0], v.length(0)).max() == 400 - short
            assert r.three.max() == 100 - short and bool(r.good.any()) == (not short)
        out.append(Case(name, "no_c0", [ref], plants, [(250, 100)], claim))
    return out


def family_far_chunk():
    out = []
    for jmod, T1, T3, ch in ((0, 450, 425, (1, 2)), (1, 450, 425, (1, 2)), (62, 450, 425, (1, 2)), (63, 450, 425, (1, 2)),
                             (50, 426, 425, (1, 2)),            # j - 499 is the LAST position of its chunk: j = 64w + 562
                             (51, 450, 425, (1, 2)),            # ... the first
                             (50, 426, 425, (2,)), (50, 426, 425, (0,)), (0, 450, 425, (0,))):
        for twin in (0, 1):
            name = f"far_chunk/j{jmod}_{T1}_{T3}_{_tag(ch)}" + ("_outside" if twin else "")
            j = 64 * 20 + jmod
            ref = synth.random_dna(synth.rng_for(_seed(name)), j + 700)
            at = j - (WINDOW - 1) - twin
            E = T1 - T3
            assert twin or at // 64 == (at + E - 1) // 64       # all in the farthest chunk the window (j - 500, j] touches
            plants = _block(0, j - T3 + 1, T3) + _block(0, at, E, ch)

            def claim(v, j=j, T1=T1, T3=T3, twin=twin):
                r = v.rows(0, T1, T3)
                if twin:
                    assert not r.good.any() and r.one.max() == T1 - 1
                else:
                    assert r.good.sum() == 1 and r.good[j] and r.one[j] == T1 and r.three[j] == T3
            out.append(Case(name, "far_chunk", [ref], plants, [(T1, T3)], claim))
    return out


def family_geometry():
    T = 425                                                    # a block of T full plants at [s, s + T): good for j in [s + 424, s + 499]
    out = []

    def add(name, L, starts, claim):
        ref = synth.random_dna(synth.rng_for(_seed(name)), L)
        plants = [p for s in starts for p in _block(0, s, T)]
        out.append(Case(name, "geometry", [ref], plants, [(T, T)], claim))

    for J in (1000, 1001, 1002):                               # start = max(1, j - 1000) at its switch point
        def claim(v, J=J):
            r = v.rows(0, T, T)
            ris, fal = _edges_of(r.good)
            assert ris.tolist() == [J] and fal.tolist() == [J + 76]
            assert (r.n_intervals, r.el) == (1, J + 76 + 1000 - max(1, J - 1000))
        add(f"geometry/rise_{J}", 3000, [J - 424], claim)
    for d in (1001, 1000, 999):                                # end = min(len, j + 1000) at its switch point
        L = 2000 + d

        def claim(v, L=L, d=d):
            r = v.rows(0, T, T)
            ris, fal = _edges_of(r.good)
            assert ris.tolist() == [1924] and fal.tolist() == [L - d]
            assert (r.n_intervals, r.el) == (1, min(L, 3000) - 924)
        add(f"geometry/fall_len-{d}", L, [1500], claim)
    for L in (2048, 2049):                                     # a run still open at the ref's end: the virtual closing edge
        def claim(v, L=L):
            r = v.rows(0, T, T)
            ris, fal = _edges_of(r.good)
            assert r.good[L - 1] and fal.tolist() == [L] and len(ris) == 1
            assert (r.n_intervals, r.el) == (1, L - max(1, int(ris[0]) - 1000))
        add(f"geometry/open_end_{L}", L, [L - 31 - T], claim)
    for g in (2499, 2500, 2501):                               # falling edge j1, rising edge j2 = j1 + g: start - prev_end = g - 2000
        j1 = 1700
        j2 = j1 + g

        def claim(v, j1=j1, j2=j2, g=g):
            r = v.rows(0, T, T)
            ris, fal = _edges_of(r.good)
            assert ris.tolist() == [j1 - 76, j2] and fal.tolist() == [j1, j2 + 76]
            assert r.n_intervals == (1 if g - 2000 < WINDOW else 2)
        add(f"geometry/gap_{g - 2000}", j2 + 76 + 1000 + 300, [1200, j2 - 424], claim)

    def claim3(v):
        r = v.rows(0, T, T)
        ris, fal = _edges_of(r.good)
        assert ris.tolist() == [1624, 4000, 6876] and fal.tolist() == [1700, 4076, 6952]
        assert (r.n_intervals, r.el) == (2, (5076 - 624) + (7952 - 5876))
    add("geometry/three_runs", 8152, [1200, 3576, 6452], claim3)
    return out


def family_many_edges():
    """T1 = T3 = 250, full plants at every even position from P0 on: every window from j = P0 + 498 on holds exactly 250.  Moving one
    plant from x to x + 1 makes j = x alone not good (two edges); the moves are 6 apart, never 500, so that none cancels another.
    The first run rises at 1998, so its start is 998 and not the clamp, and crosses a word boundary (2048) before it falls."""
    out = []
    P0 = 1500
    for target in (1022, 1024, 1026, 3002):
        name = f"many_edges/{target}"
        moves = (target - 2) // 2
        L = P0 + 600 + 6 * moves + 600
        ref = synth.random_dna(synth.rng_for(_seed(name)), L)
        moved = {P0 + 600 + 6 * k for k in range(moves)}
        plants = [(0, p + 1 if p in moved else p, ALL) for p in range(P0, L - 31, 2)]

        def claim(v, target=target, moved=moved, L=L):
            r = v.rows(0, 250, 250)
            assert r.n_edges == target
            assert not r.good[:P0 + 498].any() and r.good[P0 + 498:P0 + 600].all()
            assert not r.good[sorted(moved)].any() and r.good[P0 + 498:L - 32].sum() == L - 32 - P0 - 498 - len(moved)
            assert (r.n_intervals, r.el) == (1, L - (P0 + 498 - 1000))
        out.append(Case(name, "many_edges", [ref], plants, [(250, 250)], claim))
    return out


def family_long():
    """refs of more than 1024 words of 64 positions: the second sweep of the per-ref prefix sums, with its carry"""
    out = []
    n = 460                                                    # full plants per block: passes (450, 425)
    for L, starts in ((65536, [30000, 65536 - 31 - n]),
                      (65537, [65537 - 31 - n]),               # its only block at the very end
                      (131073, [30000, 65536 - 230, 69000, 131073 - 31 - n]),
                      (70000, [65536 - 400, 70000 - 600])):    # windows that reach back across word 1024; a block in the last 600 positions
        name = f"long/{L}"
        ref = synth.random_dna(synth.rng_for(_seed(name)), L)
        plants = [p for s in starts for p in _block(0, s, n)]

        def claim(v, L=L, starts=starts):
            r = v.rows(0, 425, 425)                           # (the all-count alone decides: chance hits are single-channel)
            ris, fal = _edges_of(r.good)
            assert ris.tolist() == [s + 424 for s in starts]
            assert fal.tolist() == [min(L, s + 500 + n - 425) for s in starts]
            assert r.three.max() == n and r.n_intervals == len(starts) and v.rows(0, 450, 425).n_intervals == len(starts)
        out.append(Case(name, "long", [ref], plants, [(425, 425), (450, 425)], claim))
    return out


def family_degenerate_db():
    out = []

    def add(name, refs, plants, claim, pairs=()):
        out.append(Case(name, "degenerate_db", refs, plants, list(pairs), claim))

    for unit, reps in ((b"A", 3000), (b"AC", 1500), (b"ACGT", 750)):           # thousands of equal entries in one fine bucket of the index
        ref = np.frombuffer(unit * reps, dtype=np.uint8)

        def claim(v):
            assert v.bits(0).all() and v.rows(0, 500, 500).good.any()
        add(f"degenerate_db/{unit.decode()}x{reps}", [ref], _block(0, 0, 3000 - 31), claim)

    rng = synth.rng_for(_seed("degenerate_db/copies"))
    orig = synth.random_dna(rng, 2500)

    def claim_copies(v):
        a, b, c = (v.rows(i, 450, 425) for i in range(3))
        assert a.good.any() and a[:2] == b[:2] and np.array_equal(a.good, b.good)
        assert np.array_equal(v.bits(2), v.bits(0)[:, ::-1]) and c.good.any()   # the same keys, mirrored
    add("degenerate_db/copies", [orig, orig.copy(), synth.revcomp(orig)], _block(0, 700, 470), claim_copies, [(450, 425)])

    def with_n(L, every, seed_name):
        s = synth.random_dna(synth.rng_for(_seed(seed_name)), L).copy()
        s[::every] = ord("N")
        return s

    no_kmer = with_n(2000, 32, "degenerate_db/n32")             # runs of 31 valid bases: no 32-mer at all

    def claim_none(v):
        assert not orc.index_ref(v.case.refs[0], coder()[1]).any() and not v.bits(0).any()
        assert v.rows(0, 0, 0)[:2] == (1, 1999) and v.rows(0, 1, 0).el == 0
    add("degenerate_db/n_every_32", [no_kmer], [], claim_none)

    n40 = with_n(2000, 40, "degenerate_db/n40")                 # runs of 39 valid bases: 8 positions in 40 have a 32-mer
    valid40 = [j for j in range(2000 - 31) if j % 40 in range(1, 9)]

    def claim_n40(v):
        assert v.bits(0).all(axis=0).nonzero()[0].tolist() == valid40
        assert v.rows(0, 104, 104).good.any() and not v.rows(0, 105, 105).good.any()      # 13 groups of 8 fit into 500 positions
    add("degenerate_db/n_every_40", [n40], [(0, j, ALL) for j in valid40], claim_n40, [(104, 104), (105, 105)])

    one = with_n(2000, 32, "degenerate_db/one")
    one[1024], one[1025] = ord("C"), ord("N")                   # bases 993 .. 1024 valid: exactly one 32-mer, at 993
    valid1 = [993]

    def claim_one(v):
        assert v.bits(0).all(axis=0).nonzero()[0].tolist() == valid1
        assert v.rows(0, 1, 1).good.sum() == WINDOW and v.rows(0, 1, 1)[:2] == (1, 2000 - 1)
    add("degenerate_db/one_kmer", [one], [(0, 993, ALL)], claim_one, [(1, 1), (2, 1)])

    lower = np.frombuffer(synth.random_dna(synth.rng_for(_seed("degenerate_db/lower")), 1800).tobytes().lower(), dtype=np.uint8)

    def claim_lower(v):
        assert v.rows(0, 450, 425).good.any() and v.rows(0, 450, 425).three.max() == 470
    add("degenerate_db/lower_case", [lower], _block(0, 600, 470), claim_lower, [(450, 425)])
    return out


FAMILIES = [family_lengths, family_exact, family_sentinel, family_no_c0, family_far_chunk, family_geometry, family_many_edges,
            family_long, family_degenerate_db]


class Catalogue:
    """every case as ONE DB in catalogue order, the planted reads, the oracle's table and bits, and the model's rows"""

    def __init__(self):
        self.header, self.cc = coder()
        self.cases = [c for fam in FAMILIES for c in fam()]
        self.refs, self.case_of = [], []
        for c in self.cases:
            c.first = len(self.refs)
            self.refs += c.refs
            self.case_of += [c] * len(c.refs)
        self.reads = [r for c in self.cases for i, j, ch in c.plants for r in plant_reads(c.refs[i], j, ch, self.cc)]
        self.table = oracle_table(self.reads, self.cc)
        self.bits = realized_bits(self.refs, self.reads, self.cc, table=self.table)
        self.pairs = sorted(set(GRID) | {p for c in self.cases for p in c.pairs})
        self._counts, self._rows = {}, {}

    def rows(self, g: int, T1: int, T3: int) -> Rows:
        key = (g, T1, T3)
        if key not in self._rows:
            if g not in self._counts:
                c, L = self.bits[g], len(self.refs[g])
                self._counts[g] = (window_counts(c[0] | c[1] | c[2], L), window_counts(c[0] & c[1] & c[2], L))
            self._rows[key] = rows_model(self.bits[g], len(self.refs[g]), T1, T3, counts=self._counts[g])
        return self._rows[key]

    def check_claim(self, case: Case):
        case.claim(View(self, case))

    def index_of(self, name: str) -> int:
        return next(c.first for c in self.cases if c.name == name)

    def db_forms(self):
        """-> {form: catalogue indices of its refs, in DB order}"""
        n = len(self.refs)
        return {"catalogue": list(range(n)), "reversed": list(range(n))[::-1],
                "single_sentinel": [self.index_of("sentinel/T377_a641")],
                "single_many_edges": [self.index_of("many_edges/1026")],
                "single_long": [self.index_of("long/131073")]}

    def reads_thrice(self):
        """the planted reads, each three times, as one read set"""
        return synth.reads_from_list(self.reads * 3)


@functools.lru_cache(maxsize=None)
def catalogue() -> Catalogue:
    return Catalogue()


def main():
    cat = catalogue()
    bad = []
    for c in cat.cases:
        try:
            cat.check_claim(c)
        except AssertionError as e:
            bad.append((c.name, e))
    print("edges: of the good bits under each case's own first pair ((450, 425) where it has none) / under (450, 425)")
    print(f"{'family':14s} {'refs':>5s} {'bases':>8s} {'plants':>7s} {'edges':>6s} {'edges(450,425)':>15s} {'reported(450,425)':>18s}")
    tot = [0, 0, 0, 0, 0, 0]
    for fam in dict.fromkeys(c.family for c in cat.cases):
        cs = [c for c in cat.cases if c.family == fam]
        gs = [c.first + i for c in cs for i in range(len(c.refs))]
        rows = [cat.rows(g, 450, 425) for g in gs]
        rep = sum(1 for g, r in zip(gs, rows) if r.el > 0 and np.float32(r.el) / np.float32(len(cat.refs[g])) > 0.75)
        own = sum(cat.rows(c.first + i, *(c.pairs[0] if c.pairs else (450, 425))).n_edges for c in cs for i in range(len(c.refs)))
        line = [len(gs), sum(len(cat.refs[g]) for g in gs), sum(len(c.plants) for c in cs), own, sum(r.n_edges for r in rows), rep]
        tot = [a + b for a, b in zip(tot, line)]
        print(f"{fam:14s} {line[0]:5d} {line[1]:8d} {line[2]:7d} {line[3]:6d} {line[4]:15d} {line[5]:18d}")
    print(f"{'total':14s} {tot[0]:5d} {tot[1]:8d} {tot[2]:7d} {tot[3]:6d} {tot[4]:15d} {tot[5]:18d}")
    print(f"reads as counted (every planted read three times): {3 * len(cat.reads)}")
    print(f"threshold pairs: {len(cat.pairs)}; stray or lost hits (realized != planted intent): {stray_hits(cat)}")
    for name, e in bad:
        print("CLAIM FAILED:", name, repr(e)[:200])
    return 1 if bad else 0


def stray_hits(cat: Catalogue) -> int:
    n = 0
    for c in cat.cases:
        for i in range(len(c.refs)):
            want = np.zeros_like(cat.bits[c.first + i])
            for k, j, ch in c.plants:
                if k == i:
                    want[list(ch), j] = True
            n += int((want != cat.bits[c.first + i]).sum())
    return n


if __name__ == "__main__":
    raise SystemExit(main())
