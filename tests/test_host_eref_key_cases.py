"""The planted-key catalogue of the eref count partition (tests/eref_key_cases.py) checked on the CPU: the coder restated in numpy
equals the oracle, every claim of every case holds at both P, every named edge value has its case, and the keys nobody planted
push nothing else over an edge."""
import numpy as np
import pytest

from oracle import binding as orc
from palace_amd import capi, synth
from tests import eref_key_cases as kc


@pytest.fixture(scope="module")
def cat():
    return kc.catalogue()


def test_keys_of_equals_the_oracle_on_random_and_planted_kmers_in_both_cases(cat):
    rng = synth.rng_for(977)
    kmers = [synth.random_dna(rng, 32) for _ in range(300)]
    for c in cat.cases[::7]:
        f = cat.form(c.name, 8)
        kmers += [f.rs.read(i) for i in range(f.rs.n) if len(f.rs.read(i)) == 32 and f.rs.read(i)[0] != ord("N")][:20]
    with_n = kmers[0].copy()
    with_n[17] = ord("N")
    kmers.append(with_n)
    for cc in (cat.cc, orc.header_to_cc(orc.header_from_picks(rng.integers(0, 6, size=32)))):
        for fold in (lambda s: s, lambda s: s | 0x20):
            arr = np.stack([fold(k) for k in kmers])
            want = np.stack([orc.index_ref(k, cc) for k in arr])
            assert np.array_equal(kc.keys_of(arr, cc), want)
    assert (kc.keys_of(np.stack(kmers[-1:]), cat.cc) == 0).all()


def test_plant_key_gives_the_key_or_none(cat):
    rng = synth.rng_for(978)
    planted = 0
    for ch in range(3):
        for key in [1, 0xffff, 1 << 25, (1 << 25) - 1, 0x12345678] + [int(x) for x in rng.integers(1, 1 << 31, size=20)]:
            r = kc.plant_key(cat.cc, ch, key, rng)
            if r is not None:
                planted += 1
                assert len(r) == 32 and orc.index_ref(r, cat.cc)[ch] == key
    assert planted > 40


def test_the_partition_arithmetic_of_the_catalogue():
    assert kc.positions_per_lane(1000, 32000) == 8 and kc.positions_per_lane(1000, 110000) == 6 and kc.positions_per_lane(0, 5) == 6
    assert kc.tile_positions(8) == 4096 and kc.tile_positions(6) == 3072
    assert kc.groups_of(0) == (0, 0) and kc.groups_of(1) == (1, 1) and kc.groups_of(5) == (1, 5) and kc.groups_of(6) == (2, 1)
    for c, cap1, sub in ((1, 1, 0), (10, 2, 0), (64, 13, 16), (92, 19, 16), (kc.BIG_CAP, 28000, 35000)):
        c1, c2 = kc.plan_caps(1 << 20, c)
        assert all(c1.cap(b) == cap1 and kc.fine_sub_cap(c2, b) == sub for b in (0, 1, 64, 127)), c
    c1, c2 = kc.plan_caps(4096, 0)
    assert c1.cap(127) >= 1024 and kc.fine_sub_cap(c2, 0) == 512 and kc.fine_sub_cap(c2, 127) == 512
    assert (capi.EREF_ROW_SLOTS, capi.EREF_GROUP_KEYS, capi.EREF_TILE2_GROUPS, capi.EREF_L1_REPLICAS, capi.EREF_BIN_THREADS, capi.EREF_XCDS,
            capi.EREF_COUNT_ROUND_VECTORS) == (72, 5, 5120, 32, 512, 8, 1024)


def test_the_constants_mirror_the_kernels_source():
    import os
    import re
    src = "".join(open(os.path.join(os.path.dirname(capi.__file__), "csrc", f)).read() for f in ("eref_common.hpp", "eref.hip"))
    for name, value in (("kRowSlots", capi.EREF_ROW_SLOTS), ("kL1Replicas", capi.EREF_L1_REPLICAS), ("kBinThreads", capi.EREF_BIN_THREADS),
                        ("kXcds", capi.EREF_XCDS), ("kGroupKeys", capi.EREF_GROUP_KEYS), ("kBin2Threads", 1024), ("kGroups2PerThread", 5),
                        ("kCountThreads", 256), ("kBatch", 4)):
        m = re.search(rf"constexpr (?:int|uint32_t) (?:[\w =,]*, )?{name} = (\d+)", src)
        assert m and int(m.group(1)) == value, name
    assert capi.EREF_TILE2_GROUPS == 1024 * 5 and capi.EREF_COUNT_ROUND_VECTORS == 4 * 256


def test_every_claim_of_every_case_holds_and_the_strays_stay_below_every_edge(cat, capsys):
    text, bad = kc.report()
    with capsys.disabled():
        print("\n" + text)
    assert not bad, [(n, P) for n, P, _ in bad]


def test_every_form_has_the_p_it_is_named_after_and_at_most_32_tiles(cat):
    for c in cat.cases:
        for P in kc.FORMS:
            f = cat.form(c.name, P)
            assert kc.positions_per_lane(f.rs.n, len(f.rs.bases)) == P
            tiles_33 = c.big or "_and_tile32" in c.name or (c.family == "rows" and P == 6 and "n128" in c.name)
            assert tiles_33 or f.n_tiles <= 32, (c.name, P, f.n_tiles)
            u, n = f.expected()
            if c.family != "regions1":                                            # (a regions1 form takes what its tile holds from a pool of reads)
                assert set(c.planted) <= set(u.tolist())                          # every planted key is a key of the read set
            if c.big:
                cat.drop(c.name)


def test_the_oracles_table_agrees_with_the_counts_of_a_form(cat):
    t = orc.CountTable()
    f = cat.form("rows/n73_x4", 6)
    t.count(f.rs.bases, f.rs.offsets, cat.cc)
    u, n = f.expected()
    assert np.array_equal(t.lookup(u), n.astype(np.uint8)) and int(n.max()) == 3
    probe = np.concatenate([u ^ np.uint32(1), u ^ np.uint32(1 << 16)])
    assert not t.lookup(probe[~np.isin(probe, u)]).any()
    t.free()


def test_every_named_edge_value_has_a_case(cat):
    names = set(cat.by_name)
    assert {f"rows/n{n}_x{m}" for n in (1, 63, 64, 65, 71, 72, 73, 74, 128) for m in (1, 2, 3, 4)} <= names
    for c, cap1 in ((1, 1), (10, 2), (64, 13)):
        for g in {cap1 - 1, cap1, cap1 + 1, 2 * cap1} - {0}:
            assert {f"regions1/c{c}_g{g}_last1", f"regions1/c{c}_g{g}_last5"} <= names
        assert {f"regions1/c{c}_g{cap1}_and_tile32", f"regions1/c{c}_g{cap1 + 1}_and_tile32"} <= names
    assert {"regions2/c64_n15", "regions2/c64_n16", "regions2/c64_n17", "regions2/c92_homeless_n90", "regions2/c1_sub_cap_0"} <= names
    assert {"count_vectors/runs_c0", "count_vectors/runs_c64", "count_vectors/overflow_only", "count_vectors/two_rounds"} <= names
    assert {f"borders/{t}_c{c}" for t in ("b0_b1", "b63_b64", "high") for c in (0, 1)} <= names
    assert {"slab/n72", "slab/n73"} <= names
    assert cat.by_name["count_vectors/two_rounds"].cap == kc.BIG_CAP and min(kc.highest_buckets()) >= 120
