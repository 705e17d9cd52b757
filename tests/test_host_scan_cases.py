"""The planted-hit catalogue of the Phase B scan (tests/scan_cases.py) against the oracle, on the CPU: the model that the device
paths are held to in test_gpu_scan_edges.py equals orc.scan_ref for every ref under every threshold pair, every case sits on the
edge it claims, and `plant` leaves exactly the channels it is asked for."""
import numpy as np
import pytest

from oracle import binding as orc
from palace_amd import synth
from tests import scan_cases as sc


@pytest.fixture(scope="module")
def cat():
    return sc.catalogue()


def test_ratio_for_gives_every_threshold_of_the_catalogue_back(cat):
    for T in sorted({t for p in cat.pairs for t in p}):
        sc.ratio_for(T)


@pytest.mark.parametrize("form", ["catalogue", "reversed"])
def test_rows_model_equals_the_oracle_for_every_ref_under_every_pair(cat, form):
    order = cat.db_forms()[form]
    assert sorted(order) == list(range(len(cat.refs)))
    idx = {g: orc.index_ref(cat.refs[g], cat.cc) for g in order}
    for T1, T3 in cat.pairs:
        r1, r3 = sc.ratio_for(T1), sc.ratio_for(T3)
        for g in order:
            L = len(cat.refs[g])
            _, n_int, el, _ = orc.scan_ref(idx[g], L, cat.table, r1, r3)
            m = cat.rows(g, T1, T3)
            assert (m.n_intervals, m.el) == (n_int, el), (cat.case_of[g].name, L, T1, T3)


def test_rows_model_stands_alone(cat):
    """the public form (bits in, rows out, nothing cached) gives what the catalogue's cached form gives"""
    for g in (cat.index_of("many_edges/1026"), cat.index_of("geometry/three_runs"), cat.index_of("lengths/0"), cat.index_of("lengths/31")):
        for T1, T3 in ((250, 250), (425, 425), (0, 0)):
            a, b = sc.rows_model(cat.bits[g], len(cat.refs[g]), T1, T3), cat.rows(g, T1, T3)
            assert a[:2] == b[:2] and a.n_edges == b.n_edges and np.array_equal(a.good, b.good)


def test_every_claim_holds(cat):
    names = [c.name for c in cat.cases]
    assert len(set(names)) == len(names)
    for c in cat.cases:
        try:
            cat.check_claim(c)
        except AssertionError as e:
            raise AssertionError(f"claim of {c.name}: {e}") from e


def test_the_catalogue_holds_what_the_device_tests_rely_on(cat):
    fams = {c.family for c in cat.cases}
    assert fams == {"lengths", "exact", "sentinel", "no_c0", "far_chunk", "geometry", "many_edges", "long", "degenerate_db"}
    assert [len(c.refs[0]) for c in cat.cases if c.family == "lengths"] == sc.LENGTHS
    assert set(sc.GRID) <= set(cat.pairs)
    assert sum(len(r) for r in cat.refs) < 1_000_000 and 3 * len(cat.reads) < 500_000
    n_edges = {c.name: cat.rows(c.first, 250, 250).n_edges for c in cat.cases if c.family == "many_edges"}
    assert sorted(n_edges.values()) == [1022, 1024, 1026, 3002]            # around the 1024 edges the window kernel's list holds
    assert max(len(r) for r in cat.refs) > 2 * 65536                         # three sweeps of 1024 words


def test_plant_gives_exactly_the_wanted_subset():
    cc = sc.coder()[1]
    rng = synth.rng_for(4242)
    ref = synth.random_dna(rng, 3000)
    subsets = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
    draws = [(int(j), subsets[int(k)]) for j, k in zip(rng.choice(3000 - 31, size=200, replace=False), rng.integers(0, 7, size=200))]
    reads = []
    for j, ch in draws:
        got = sc.plant_reads(ref, j, ch, cc)
        assert (len(got) == 1 or len(ch) == 2) and all(r.shape == (32,) for r in got)
        if len(ch) != 2:
            assert np.array_equal(got[0], sc.plant(ref, j, ch, cc)) and int((got[0] != ref[j:j + 32]).sum()) == (len(ch) == 1)
        reads += got
    bits = sc.realized_bits([ref], reads, cc)[0]
    want = np.zeros_like(bits)
    for j, ch in draws:
        want[list(ch), j] = True
    assert np.array_equal(bits, want)
    with pytest.raises(ValueError):
        n = ref.copy()
        n[100] = ord("N")
        sc.plant(n, 90, (0,), cc)
