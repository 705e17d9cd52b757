"""Planted keys at the capacity edges of the eref count partition (Phase A: level 1, level 2, count kernel) -- no GPU needed.

Every other count test takes random or skewed reads and lets chance decide which keys meet a full staging row, a full region or a
partly valid vector.  Here the keys are PLANTED: channel i's forward index takes bit 31 - z from one projection of base z alone
and every projection bit is offered by two of the four bases, so any 32-bit K has 2^32 32-mers whose forward index in channel i
is K; the free choices move the reverse-complement index, and `plant_key` tries random ones until rc >= K -- a 32-base read whose
canonical channel-i key is exactly K.  Such a read has ONE position, so a read set of them is laid out key by key:

  * a level-1 workgroup takes one tile of 512 * P positions (128 planted reads for P = 8, 96 for P = 6) and writes to replica
    tile % 32 of every bucket; up to 32 tiles, every tile's run of a bucket lies alone at group 0 of its own region, and the
    level-2 workgroup of that region sees exactly that run (with more tiles, the runs of tiles t, t + 32, ... share a region);
  * how many keys a staging row, a level-1 region or a fine sub-region receives follows from the keys in position order; the
    order atomics land in and the XCD a workgroup runs on change WHICH key takes a slow path, never how many do.

P follows the mean read length (`positions_per_lane`): the P = 8 form of a case fills its gaps with 32-base reads of N, the
P = 6 form with long ones (no N read makes a key).

The planted intent is never the expectation: that is `Form.counts`, orc.index_ref over the whole read set (cut to a share's
buckets where a run counts a share of the key space).  A case carries a CLAIM over the realized keys (such as "row 300 of
bucket 1 receives exactly 73 keys in tile 0 and no other row more than 64") which shows that the input sits on the edge it is
named after; claims are asserted, never filtered -- a case whose claim fails is repaired here (SEED_BUMP).  Keys that do not
plant within PLANT_TRIES are replaced while the case is built, never skipped by a test.

    python -m tests.eref_key_cases        # per family: the cases, their forms, the planted keys and the claims
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, field
from typing import Callable

import numpy as np

from oracle import binding as orc
from palace_amd import capi, synth
from tests import scan_cases

PLANT_TRIES = 4000
FORMS = (8, 6)                                   # positions per lane of the level-1 kernel
L1_SHIFT, FINE_SHIFT, L1_BUCKETS, L2_ROWS = 25, 16, 128, 512
SLAB = 64 * 1024                                 # option slab_bases of the `slab` family
BIG_CAP = 140000                                 # the bucket_cap test_binned_path_equals_oracle uses
SEED_BUMP: dict = {}

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.array([[1, 0, 0, 1], [1, 1, 0, 0], [1, 0, 1, 0]], np.uint64)      # projection q of A, C, G, T: {A,T}, {A,C}, {A,G}
_COMP = np.array([3, 2, 1, 0])                                               # A <-> T, C <-> G
_Z = np.arange(32, dtype=np.uint64)


def coder():
    return scan_cases.coder()


# ---- the coder, restated ------------------------------------------------------------------------------------------------
def fwd_rc_of(kmers, cc):
    """-> (fwd[n, 3], rc[n, 3], valid[n]) of n 32-mers (ASCII, either case) under choose_coder[96]: channel i reads projection
    cc[3 z + i] of base z with weight 2^(31 - z); the reverse complement reads cc[3 (31 - z) + i] of the complement, weight 2^z"""
    k = np.asarray(kmers, np.uint8).reshape(-1, 32)
    up = k & 0xDF
    idx = np.full(up.shape, -1, np.int64)
    for b, ch in enumerate(b"ACGT"):
        idx[up == ch] = b
    valid = (idx >= 0).all(axis=1)
    idx = np.where(idx < 0, 0, idx)
    q = np.asarray(cc, np.int64).reshape(32, 3)
    fwd, rc = np.zeros((len(k), 3), np.uint64), np.zeros((len(k), 3), np.uint64)
    for i in range(3):
        fwd[:, i] = (_CODE[q[:, i][None, :], idx] << (np.uint64(31) - _Z)).sum(axis=1)
        rc[:, i] = (_CODE[q[::-1, i][None, :], _COMP[idx]] << _Z).sum(axis=1)
    return fwd, rc, valid


def keys_of(kmers, cc) -> np.ndarray:
    """canonical keys [n, 3] of n 32-mers; 0 where a base is none of ACGTacgt (as orc.index_ref reports it)"""
    fwd, rc, valid = fwd_rc_of(kmers, cc)
    out = np.minimum(fwd, rc).astype(np.uint32)
    out[~valid] = 0
    return out


def plant_key(cc, channel: int, key: int, rng, tries: int = PLANT_TRIES, accept: Callable | None = None):
    """32 bases whose canonical channel-`channel` key is `key`, or None after `tries` random choices of the free bits.
    accept(keys[n, 3]) -> bool[n] narrows the choice further (by the read's other two keys)."""
    q = np.asarray(cc, np.int64).reshape(32, 3)[:, channel]
    bits = (np.uint64(key) >> (np.uint64(31) - _Z)) & np.uint64(1)
    opts = np.array([[b for b in range(4) if _CODE[q[z], b] == bits[z]] for z in range(32)])      # the two bases per offset
    done = 0
    while done < tries:
        n = min(256, tries - done)
        done += n
        kmers = _ACGT[opts[np.arange(32)[None, :], rng.integers(0, 2, size=(n, 32))]]
        fwd, rc, _ = fwd_rc_of(kmers, cc)
        assert (fwd[:, channel] == key).all()
        good = rc[:, channel] >= np.uint64(key)
        if accept is not None:
            good &= accept(np.minimum(fwd, rc).astype(np.uint32))
        if good.any():
            return kmers[int(np.flatnonzero(good)[0])].copy()
    return None


# ---- the partition's arithmetic (csrc/eref.hip, csrc/eref_common.hpp), used for claims only ------------------------------------
def positions_per_lane(n_reads: int, n_positions: int) -> int:
    """bin_and_count's P from count_reads_from's key density"""
    kpp = 3.0 * max(0.02, 1.0 - 31.0 * n_reads / max(1.0, float(n_positions))) if n_reads else 3.0
    return 6 if kpp > 1.6 else 8


def tile_positions(P: int) -> int:
    return capi.EREF_BIN_THREADS * P


def reads_per_tile(P: int) -> int:
    return tile_positions(P) // 32


def l1_bucket(key):
    return np.asarray(key, np.uint32) >> L1_SHIFT


def fine_row(key):
    return (np.asarray(key, np.uint32) >> FINE_SHIFT) & (L2_ROWS - 1)


def groups_of(n_keys: int):
    """-> (groups of a run of n_keys keys, keys in its last group)"""
    g = -(-n_keys // capi.EREF_GROUP_KEYS)
    return g, n_keys - (g - 1) * capi.EREF_GROUP_KEYS if g else 0


@dataclass
class DensityCaps:
    share: int
    pad: int
    unit: int = 4

    def prefix(self, b: int) -> int:
        return self.unit * (self.pad * b + ((self.share * (b * (256 - b))) >> 7))

    def cap(self, b: int) -> int:
        return self.prefix(b + 1) - self.prefix(b)


def plan_caps(slab_positions: int, cap_override: int):
    """plan_count's (caps1 in groups per level-1 region, caps2 in pairs of keys per fine bucket) for a slab of slab_positions"""
    if cap_override > 0:
        return (DensityCaps(0, -(-cap_override // capi.EREF_GROUP_KEYS), 1), DensityCaps(0, (cap_override + 3) // 4))
    max_keys = 3 * slab_positions
    mean1 = max_keys // (L1_BUCKETS * capi.EREF_L1_REPLICAS) // capi.EREF_GROUP_KEYS * 26 // 25 + 1
    mean2 = max_keys // (1 << FINE_SHIFT) // 2
    return (DensityCaps(mean1 + mean1 // 5, mean1 // 8 + 1024, 1), DensityCaps((mean2 + mean2 // 5) // 4, (mean2 // 8 + 2048) // 4))


def fine_sub_cap(caps2: DensityCaps, b1: int) -> int:
    return (2 * caps2.cap(b1) // capi.EREF_XCDS) & ~7


# ---- read sets laid out key by key -------------------------------------------------------------------------------------------
def n_read(length: int) -> np.ndarray:
    return np.full(length, ord("N"), np.uint8)


def lay_out(placement, P: int) -> synth.ReadSet:
    """placement: [(first position, reads)] -> the read set with every block at its position; the gaps are N reads of 32 bases
    (P = 8) or one long N read each plus a tail (P = 6: mean read length above 66)"""
    reads, cur = [], 0
    for at, block in sorted(placement, key=lambda x: x[0]):
        gap = at - cur
        assert gap >= 0, "blocks overlap"
        if P == 8:
            reads += [n_read(32)] * (gap // 32) + ([n_read(gap % 32)] if gap % 32 else [])
        elif gap:
            reads.append(n_read(gap))
        reads += list(block)
        cur = at + sum(len(r) for r in block)
    if P == 6 and 67 * (len(reads) + 1) > cur:
        reads.append(n_read(67 * (len(reads) + 1) - cur))
    rs = synth.reads_from_list(reads)
    assert positions_per_lane(rs.n, len(rs.bases)) == P, (P, rs.n, len(rs.bases))
    return rs


@dataclass
class Case:
    name: str
    family: str
    cap: int                                 # bucket_cap of palace_eref_set_count_mode(2, cap); 0: the plan's own capacities
    buckets: tuple                           # the level-1 buckets the case plants in: the share, and its complement
    place: Callable                          # place(P) -> placement for lay_out
    claim: Callable                          # claim(form): asserts what makes this case the edge it is named after
    edge: str                                # the claim in words
    planted: list = field(default_factory=list)      # the keys planted in channel 0
    targets: frozenset = frozenset()         # fine buckets (key >> 16) planted on purpose: free to pass 64 keys of a row / the sub-region
    slab: int = 0                            # option slab_bases
    big: bool = False                        # more than 32 tiles, claim on the key total only


class Form:
    """a case at one P: the read set, its realized keys (orc.index_ref over the whole set, every channel) by position, and
    where the partition puts them"""

    def __init__(self, case: Case, P: int):
        self.case, self.P = case, P
        self.rs = lay_out(case.place(P), P)
        cc = coder()[1]
        bases, off = self.rs.bases, self.rs.offsets
        idx = orc.index_ref(bases, cc).reshape(-1, 3)
        end_of = np.repeat(off[1:], np.diff(off))[:len(idx)]
        inside = np.arange(len(idx)) + 32 <= end_of                          # the 32-mer lies in one read
        sel = inside[:, None] & (idx != 0)
        self.pos = np.nonzero(sel)[0]
        self.key = idx[sel]
        slab = case.slab or max(64, -(-len(bases) // 64) * 64)
        self.slab_of = self.pos // slab
        self.tile = (self.pos - self.slab_of * slab) // tile_positions(P)
        self.n_slabs = -(-len(bases) // slab)
        self.n_tiles = -(-min(len(bases), slab) // tile_positions(P))       # of the fullest slab
        self.caps1, self.caps2 = plan_caps(min(len(bases), slab), case.cap)
        u, c = np.unique(self.key, return_counts=True)
        self.counts = (u, np.minimum(c, 3))

    def expected(self, buckets=None, times: int = 1):
        """the oracle's (keys, min(3, times * multiplicity)), cut to `buckets` (None: the whole key space)"""
        u, c = np.unique(self.key, return_counts=True)
        if buckets is not None:
            m = np.isin(u >> L1_SHIFT, list(buckets))
            u, c = u[m], c[m]
        return u, np.minimum(times * c, 3)

    def cap1(self, b: int) -> int:
        return self.caps1.cap(b)

    def sub_cap(self, b: int) -> int:
        return fine_sub_cap(self.caps2, b)

    def run(self, bucket: int, tile: int, slab: int = 0):
        """-> (keys, groups, keys of the last group) of the run level-1 tile `tile` writes for `bucket`"""
        n = int(((self.key >> L1_SHIFT == bucket) & (self.tile == tile) & (self.slab_of == slab)).sum())
        return (n,) + groups_of(n)

    def unit_fine(self, replica: int, slab: int = 0):
        """-> (fine buckets, key counts) of everything the level-1 tiles of one replica hand to level 2"""
        m = (self.tile % capi.EREF_L1_REPLICAS == replica) & (self.slab_of == slab)
        return np.unique(self.key[m] >> FINE_SHIFT, return_counts=True)

    def row_keys(self, fine: int, replica: int, slab: int = 0) -> int:
        f, c = self.unit_fine(replica, slab)
        return int(c[f == fine].sum())

    def fine_runs(self, fine: int):
        """-> {(slab, tile): keys} of one fine bucket"""
        m = self.key >> FINE_SHIFT == fine
        out: dict = {}
        for s, t in zip(self.slab_of[m].tolist(), self.tile[m].tolist()):
            out[(s, t)] = out.get((s, t), 0) + 1
        return out

    def region_groups(self):
        """-> {(slab, bucket, replica): groups reserved in that level-1 region}"""
        comb = (self.slab_of * (1 << 20) + self.tile) * L1_BUCKETS + (self.key >> L1_SHIFT).astype(np.int64)
        u, c = np.unique(comb, return_counts=True)
        out: dict = {}
        for x, n in zip(u.tolist(), c.tolist()):
            st, b = divmod(x, L1_BUCKETS)
            s, t = divmod(st, 1 << 20)
            k = (s, b, t % capi.EREF_L1_REPLICAS)
            out[k] = out.get(k, 0) + groups_of(n)[0]
        return out


def check_strays(form: Form):
    """the keys nobody planted on purpose (channels 1 and 2 of the planted reads) push no second row, region or sub-region over its
    edge: outside the case's targets no staging row passes 64 keys, no fine bucket its sub-region, and outside its buckets no
    level-1 region its capacity"""
    case = form.case
    if case.big:
        return
    for (s, b, r), g in form.region_groups().items():
        assert g <= capi.EREF_TILE2_GROUPS, (case.name, "a region of more than one level-2 tile", s, b, r, g)
        if b not in case.buckets:
            assert g <= form.cap1(b), (case.name, "a stray region overflows", s, b, r, g)
    for s in range(form.n_slabs):
        for r in range(min(form.n_tiles, capi.EREF_L1_REPLICAS)):
            f, c = form.unit_fine(r, s)
            stray = ~np.isin(f, list(case.targets))
            assert not (c[stray] > 64).any(), (case.name, "a stray row passes 64 keys", s, r)
    f, c = np.unique(form.key >> FINE_SHIFT, return_counts=True)
    for fine, n in zip(f.tolist(), c.tolist()):
        sc = form.sub_cap(fine >> 9)
        if fine not in case.targets and sc:
            assert n <= sc, (case.name, "a stray fine bucket passes its sub-region", fine, n)


# ---- planting ----------------------------------------------------------------------------------------------------------------
def _rng(name):
    return synth.rng_for(zlib.crc32(name.encode()) + SEED_BUMP.get(name, 0))


def _none_in(buckets):
    """accept: neither stray key (channels 1, 2) falls into one of `buckets`"""
    bs = np.array(sorted(buckets), np.uint32)
    return lambda k: ~np.isin(k[:, 1:] >> L1_SHIFT, bs).any(axis=1)


def _exactly_one_in(bucket):
    return lambda k: ((k[:, 1:] >> L1_SHIFT) == bucket).sum(axis=1) == 1


def plant_fine(rng, fine: int, n: int, accept, lows=(0, 1, 31, 32, 0xffff, 0xfffe, 0x8000, 0x7fff)):
    """n reads with n distinct channel-0 keys of fine bucket `fine`: the low 16 bits from `lows` first (word and slice edges of
    the count kernel), then random; a key that does not plant is replaced by the next -> (keys, reads)"""
    cc = coder()[1]
    keys, reads, seen = [], [], set()
    cand = [x for x in lows if (fine << FINE_SHIFT) | x]
    while len(keys) < n:
        x = cand.pop(0) if cand else int(rng.integers(0, 1 << 16))
        if x in seen:
            continue
        seen.add(x)
        key = (fine << FINE_SHIFT) | x
        r = plant_key(cc, 0, key, rng, accept=accept)
        if r is not None:
            keys.append(key)
            reads.append(r)
        assert len(seen) < 4 * n + 64, "fine bucket does not plant"
    return keys, reads


def plant_in_bucket(rng, bucket: int, n: int, accept):
    """n reads with distinct channel-0 keys spread over the rows of level-1 bucket `bucket` -> (keys, reads)"""
    cc = coder()[1]
    keys, reads = [], []
    while len(keys) < n:
        key = (bucket << L1_SHIFT) | int(rng.integers(1, 1 << L1_SHIFT))
        r = None if key in keys else plant_key(cc, 0, key, rng, accept=accept)
        if r is not None:
            keys.append(key)
            reads.append(r)
    return keys, reads


def _tile_at(t, P):
    return t * tile_positions(P)


def _in_tiles(blocks):
    """blocks: [(tile, reads)] -> place(P); a block longer than a tile holds goes on in the tile 32 later (the same replica)"""
    def place(P):
        out, per = [], reads_per_tile(P)
        for t, reads in blocks:
            for j in range(0, len(reads), per):
                out.append((_tile_at(t + capi.EREF_L1_REPLICAS * (j // per), P), reads[j:j + per]))
        return out
    return place


# ---- the families ------------------------------------------------------------------------------------------------------------
ROW_N = (1, 63, 64, 65, 71, 72, 73, 74, 128)


def family_rows():
    """one staging row of level 2 at its edges: 64 (second flush pass), 72 (full), 73 (the first homeless key)"""
    out = []
    bucket, row = 1, 300
    fine = bucket * L2_ROWS + row
    for n in ROW_N:
        for copies in (1, 2, 3, 4):
            name = f"rows/n{n}_x{copies}"
            keys, reads = plant_fine(_rng(name), fine, n, _none_in({bucket}))

            def claim(f, n=n, copies=copies):
                assert f.n_tiles <= 32 or n > reads_per_tile(f.P)
                for t in range(copies):
                    assert f.row_keys(fine, t) == n, (t, f.row_keys(fine, t))
                    ff, c = f.unit_fine(t)
                    assert not (c[ff != fine] > 64).any()
                    assert sum(f.run(bucket, t + 32 * j)[1] for j in range(2)) <= min(f.cap1(bucket), capi.EREF_TILE2_GROUPS)
                assert n * copies <= f.sub_cap(bucket)             # nothing leaves the partition's fast paths but the homeless keys
            out.append(Case(name, "rows", 0, (bucket,), _in_tiles([(t, reads) for t in range(copies)]), claim,
                            f"row {row} of bucket {bucket} receives exactly {n} keys in each of {copies} tile(s), no other row more than 64",
                            keys, frozenset({fine})))
    return out


def family_regions1():
    """one level-1 region at its capacity: cap1 - 1, cap1, cap1 + 1 and 2 cap1 groups, the last group with 1 key and with 5"""
    out = []
    bucket = 0
    for c in (1, 10, 64):
        cap1 = -(-c // capi.EREF_GROUP_KEYS)
        for g in sorted({cap1 - 1, cap1, cap1 + 1, 2 * cap1} - {0}):
            for last in (1, 5):
                name = f"regions1/c{c}_g{g}_last{last}"
                k = capi.EREF_GROUP_KEYS * (g - 1) + last
                rng = _rng(name)
                keys1, singles = plant_in_bucket(rng, bucket, k, _none_in({bucket}))
                # more keys than a tile holds reads: reads whose channel-1 or channel-2 key lies in the bucket as well
                keys2, doubles = plant_in_bucket(rng, bucket, max(0, k - reads_per_tile(6)), _exactly_one_in(bucket))

                def place(P, singles=singles, doubles=doubles, k=k):
                    nd = max(0, k - reads_per_tile(P))
                    return [(0, doubles[:nd] + singles[:k - 2 * nd])]

                def claim(f, g=g, last=last, cap1=cap1, k=k):
                    assert f.cap1(bucket) == cap1 and f.n_tiles <= 32
                    assert f.run(bucket, 0) == (k, g, last), f.run(bucket, 0)
                out.append(Case(name, "regions1", c, (bucket,), place, claim,
                                f"bucket {bucket}'s run of tile 0 holds {g} groups, the last {last} key(s), against a region of {cap1}",
                                keys1 + keys2))
        for ga in (cap1, cap1 + 1):
            name = f"regions1/c{c}_g{ga}_and_tile32"
            rng = _rng(name)
            ka, kb = capi.EREF_GROUP_KEYS * (ga - 1) + 3, capi.EREF_GROUP_KEYS * (cap1 - 1) + 2
            keys_a, reads_a = plant_in_bucket(rng, bucket, ka, _none_in({bucket}))
            keys_b, reads_b = plant_in_bucket(rng, bucket, kb, _none_in({bucket}))

            def claim(f, ga=ga, cap1=cap1, ka=ka, kb=kb):
                assert f.cap1(bucket) == cap1 and f.n_tiles == 33
                assert f.run(bucket, 0) == (ka, ga, 3) and f.run(bucket, 32) == (kb, cap1, 2)      # whichever reserves second starts at >= cap1
            out.append(Case(name, "regions1", c, (bucket,), _in_tiles([(0, reads_a), (32, reads_b)]), claim,
                            f"tiles 0 and 32 (one replica) write runs of {ga} and {cap1} groups into a region of {cap1}: the second starts at or behind its end",
                            keys_a + keys_b))
    return out


def family_regions2():
    """one row's run against its XCD sub-region"""
    out = []
    bucket, row = 1, 200
    fine = bucket * L2_ROWS + row

    def add(name, c, n, tiles, claim, edge):
        keys, reads = plant_fine(_rng(name), fine, n, _none_in({bucket}))
        out.append(Case(name, "regions2", c, (bucket,), _in_tiles([(t, reads) for t in range(tiles)]), claim, edge, keys, frozenset({fine})))

    for n in (15, 16, 17):
        def claim(f, n=n):
            assert f.sub_cap(bucket) == 16 and f.fine_runs(fine) == {(0, 0): n}
            assert f.run(bucket, 0)[1] <= f.cap1(bucket)
        add(f"regions2/c64_n{n}", 64, n, 1, claim, f"a run of {n} keys against a sub-region of 16")

    def claim_homeless(f):
        assert f.sub_cap(bucket) == 16 and f.fine_runs(fine) == {(0, 0): 90}
        assert f.run(bucket, 0)[1] <= f.cap1(bucket)               # all 90 reach level 2: 72 staged, 18 homeless, 16 of them fit
        assert 90 - capi.EREF_ROW_SLOTS > f.sub_cap(bucket)
    add("regions2/c92_homeless_n90", 92, 90, 1, claim_homeless, "90 keys of one row: 18 homeless keys against a sub-region of 16, then the staged 72 against a full one")

    def claim_zero(f):
        assert f.sub_cap(bucket) == 0 and f.cap1(bucket) == 1
        assert f.fine_runs(fine) == {(0, t): 3 for t in range(4)} and all(f.run(bucket, t)[1] == 1 for t in range(4))
    add("regions2/c1_sub_cap_0", 1, 3, 4, claim_zero, "sub_cap = 0: the one group that fits every region is marked key by key at level 2")
    return out


def family_count_vectors():
    """the count kernel's walk: partly valid last vectors, a bucket of overflow keys only, a second round of the batch loop"""
    out = []
    bucket, row = 1, 100
    fine = bucket * L2_ROWS + row
    sizes = (1, 7, 8, 9, 15)
    for c in (0, 64):
        name = f"count_vectors/runs_c{c}"
        keys, reads = plant_fine(_rng(name), fine, sum(sizes), _none_in({bucket}))
        blocks, at = [], 0
        for t, n in enumerate(sizes):
            blocks.append((t, reads[at:at + n]))
            at += n
        blocks.append((len(sizes), reads[at - 15:at]))                          # the last run once more: counts of 2

        def claim(f):
            assert f.fine_runs(fine) == {(0, t): n for t, n in enumerate(sizes + (15,))}
            assert f.sub_cap(bucket) >= 16 and all(f.run(bucket, t)[1] <= f.cap1(bucket) for t in range(6))
        out.append(Case(name, "count_vectors", c, (bucket,), _in_tiles(blocks), claim,
                        "six tiles (six level-2 workgroups) bring runs of 1, 7, 8, 9, 15 and 15 keys to one fine bucket", keys, frozenset({fine})))

    name = "count_vectors/overflow_only"
    keys, reads = plant_fine(_rng(name), fine, 7, _none_in({bucket}))

    def claim_over(f):
        assert f.sub_cap(bucket) == 0 and f.run(bucket, 0) == (7, 2, 2) and f.cap1(bucket) == 1     # n8 == 0 everywhere, the bucket touched
    out.append(Case(name, "count_vectors", 1, (bucket,), _in_tiles([(0, reads), (1, reads[:4]), (2, reads[:2])]), claim_over,
                    "seven keys of one fine bucket, none in a sub-region: five marked at level 2, two at level 1", keys, frozenset({fine})))

    name = "count_vectors/two_rounds"
    rng = _rng(name)
    keys, reads = plant_fine(rng, fine, 65, _none_in({bucket}))
    repeats = capi.EREF_COUNT_ROUND_VECTORS * 8 + 200

    def place(P):
        every = repeats // 64
        seq = []
        for i in range(repeats):
            seq.append(reads[0])
            if i % every == every - 1 and i // every < 64:
                seq.append(reads[1 + i // every])
        return [(0, seq)]

    def claim_big(f):
        assert sum(f.fine_runs(fine).values()) == repeats + 64 > capi.EREF_COUNT_ROUND_VECTORS * 8
        assert f.n_tiles > 32 and f.sub_cap(bucket) >= repeats + 64
    out.append(Case(name, "count_vectors", BIG_CAP, (bucket,), place, claim_big,
                    f"one read {repeats} times and 64 others of its fine bucket: more than {capi.EREF_COUNT_ROUND_VECTORS} vectors", keys, frozenset({fine}),
                    big=True))
    return out


def _end_row_lows(rng, extra: int):
    return [0, 1, 0xfffe, 0xffff] + [int(x) for x in rng.integers(2, 0xfffe, size=extra)]


@functools.lru_cache(maxsize=None)
def highest_buckets():
    """the two highest level-1 buckets in whose first AND last fine row a key plants: canonical keys thin out towards 2^32, and
    where the coder reads offsets z and 31 - z through one projection the key itself fixes a bit of its reverse complement"""
    cc, rng, found = coder()[1], _rng("borders/highest"), []
    for b in range(L1_BUCKETS - 1, 64, -1):
        if all(any(plant_key(cc, 0, (b << L1_SHIFT) | (r << FINE_SHIFT) | x, rng) is not None for x in _end_row_lows(rng, 12)[2:])
               for r in (0, L2_ROWS - 1)):
            found.append(b)
            if len(found) == 2:
                return tuple(found)
    raise AssertionError("no high bucket plants")


def family_borders():
    """keys at the ends of the level-1 buckets and of the key space"""
    out = []
    cc = coder()[1]
    hi = highest_buckets()
    for tag, bs in (("b0_b1", (0, 1)), ("b63_b64", (63, 64)), ("high", tuple(sorted(hi)))):
        want = []
        for b in bs:
            for r in (0, L2_ROWS - 1):
                want += [(b << L1_SHIFT) | (r << FINE_SHIFT) | x for x in _end_row_lows(_rng(f"borders/{tag}/{b}/{r}"), 16 if tag == "high" else 0)]
        want = [k for k in want if 0 < k < (1 << 32) - 1]
        for c in (0, 1):
            name = f"borders/{tag}_c{c}"
            rng = _rng(name)
            keys, reads, mult = [], [], {}
            for i, k in enumerate(want):
                for _ in range(1 + i % 3):                                       # every key once, twice or three times, by different reads
                    r = plant_key(cc, 0, k, rng, accept=_none_in(set(bs)))
                    if r is not None:
                        reads.append(r)
                        mult[k] = mult.get(k, 0) + 1
                if k in mult:
                    keys.append(k)

            def claim(f, bs=bs, mult=dict(mult), tag=tag):
                u, n = f.expected()
                got = dict(zip(u.tolist(), n.tolist()))
                assert all(got.get(k) == m for k, m in mult.items())
                rows = {(k >> L1_SHIFT, (k >> FINE_SHIFT) & 511) for k in mult}
                assert all((b, r) in rows for b in bs for r in (0, L2_ROWS - 1)), rows            # both end rows of every bucket planted
                if tag == "b0_b1":
                    assert {1, (1 << 25) - 1, 1 << 25} <= set(mult)
                if tag == "b63_b64":
                    assert {(64 << 25) - 1, 64 << 25} <= set(mult)
                if tag == "high":
                    assert min(bs) >= 120
            blocks = [(t, reads[8 * t:8 * t + 8]) for t in range(-(-len(reads) // 8))]      # eight to a tile: a region of one group holds the strays
            out.append(Case(name, "borders", c, bs, _in_tiles(blocks), claim,
                            f"keys in the first and the last fine row of buckets {bs}, the last key of one beside the first of the next",
                            keys, frozenset(k >> FINE_SHIFT for k in keys)))
    return out


def family_slab():
    """a `rows` case cut by a slab edge: the second slab's first tile holds the full row, the first slab's last tile more of it"""
    out = []
    bucket, row, before = 1, 400, 30
    fine = bucket * L2_ROWS + row
    for n in (72, 73):
        name = f"slab/n{n}"
        keys, reads = plant_fine(_rng(name), fine, n + before, _none_in({bucket}))

        def place(P, reads=reads):
            return [(SLAB - 32 * before, reads)]

        def claim(f, n=n):
            last = (SLAB - 1) // tile_positions(f.P)
            assert f.fine_runs(fine) == {(0, last): before, (1, 0): n} and f.n_slabs >= 2
        out.append(Case(name, "slab", 0, (bucket,), place, claim,
                        f"slabs of {SLAB} positions: row {row} receives {before} keys in the first slab's last tile and {n} in the second slab's first",
                        keys, frozenset({fine}), slab=SLAB))
    return out


FAMILIES = [family_rows, family_regions1, family_regions2, family_count_vectors, family_borders, family_slab]


class Catalogue:
    def __init__(self):
        self.header, self.cc = coder()
        self.cases = [c for fam in FAMILIES for c in fam()]
        self.by_name = {c.name: c for c in self.cases}
        assert len(self.by_name) == len(self.cases)
        self._forms: dict = {}

    def form(self, name: str, P: int) -> Form:
        if (name, P) not in self._forms:
            self._forms[(name, P)] = Form(self.by_name[name], P)
        return self._forms[(name, P)]

    def drop(self, name: str):
        for P in FORMS:
            self._forms.pop((name, P), None)


@functools.lru_cache(maxsize=None)
def catalogue() -> Catalogue:
    return Catalogue()


def report() -> tuple:
    """-> (text, failed claims)"""
    cat = catalogue()
    lines, bad = [], []
    for fam in dict.fromkeys(c.family for c in cat.cases):
        lines.append(f"== {fam}")
        for c in (c for c in cat.cases if c.family == fam):
            forms = []
            for P in FORMS:
                f = cat.form(c.name, P)
                try:
                    c.claim(f)
                    check_strays(f)
                    ok = "ok"
                except AssertionError as e:
                    ok = "CLAIM FAILED"
                    bad.append((c.name, P, e))
                forms.append(f"P={P}: {f.rs.n} reads, {len(f.rs.bases)} bases, {f.n_slabs}x{f.n_tiles} tiles, {len(f.key)} keys, {ok}")
                if c.big:
                    cat.drop(c.name)
            ks = " ".join(f"{k:08x}" for k in c.planted[:4]) + (" ..." if len(c.planted) > 4 else "")
            lines.append(f"{c.name:34s} cap {c.cap:6d} buckets {c.buckets}  planted {len(c.planted):3d} keys: {ks}")
            lines.append(f"{'':34s} claim: {c.edge}")
            lines += [f"{'':34s} {x}" for x in forms]
    lines.append(f"{len(cat.cases)} cases; highest buckets that plant: {highest_buckets()}")
    for name, P, e in bad:
        lines.append(f"CLAIM FAILED: {name} P={P} {e!r}"[:300])
    return "\n".join(lines), bad


def main():
    text, bad = report()
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
