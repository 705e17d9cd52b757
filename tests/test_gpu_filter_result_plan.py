"""palace_filter_result_plan and palace_paths_first_of_equal (csrc/filter_result.hip) at the C ABI against the restatement of
tests/filter_result_cases.py (path_class, first_of_equal): some 5 000 random paths of 1, 2, 64, 65 and 1 500 tokens over 200 records
with random bits and tags, the decision's edges by hand, and the first-occurrence rule on 4 000 copies of one path, paths equal up to
the last token, the same names on another strand and a prefix of another path -- each at hash_bits 64 and 3 (where nearly every
path collides), with identical results."""
import numpy as np
import pytest

from palace_amd import capi
from tests import filter_result_cases as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def expected(code, path_off, tags, rec_len, rec_bits):
    cls, all_len = [], []
    for p in range(len(path_off) - 1):
        recs = [c >> 2 for c in code[path_off[p]:path_off[p + 1]] if c >= 0 and not c & 2]
        bits = 0
        for r in recs:
            bits |= int(rec_bits[r])
        total = sum(int(rec_len[r]) for r in recs)
        hit = sum(int(rec_len[r]) for r in recs if rec_bits[r] & fr.REC_BLAST)
        cls.append(fr.path_class(int(path_off[p + 1] - path_off[p]), int(tags[p]), bool(bits & fr.REC_GENE), bool(bits & fr.REC_S07), bool(bits & fr.REC_S09), total, hit))
        all_len.append(total)
    return np.array(cls, np.uint8), np.array(all_len, np.int64)


def run_plan(ctx, paths, tags, rec_len, rec_bits):
    code = np.array([c for p in paths for c in p], np.int32)
    path_off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    fp = capi.FilterPlan(ctx, code, path_off, rec_len)
    try:
        got = fp.plan(tags, rec_bits)
    finally:
        fp.free()
    want = expected(code, path_off, tags, rec_len, rec_bits)
    assert (got[1] == want[1]).all()
    assert (got[0] == want[0]).all(), np.flatnonzero(got[0] != want[0])[:10]
    return got[0]


def test_random_paths(ctx):
    rng = np.random.default_rng(41)
    rec_len = rng.choice([0, 1, 4, 5, 100, 250, 999, 1000, 5000], size=200)
    rec_bits = rng.choice([0, 0, 0, 0, 1, 2, 6, 8, 8, 9, 14, 15], size=200).astype(np.uint8)
    paths = [[]]
    for n, count in ((1, 2500), (2, 1500), (64, 500), (65, 500), (1500, 12)):
        for _ in range(count):
            p = (rng.integers(0, 200, size=n) << 2 | rng.integers(0, 2, size=n)).astype(np.int64)
            bad = rng.random(n) < 0.03
            p[bad] = rng.choice([-1, -2, 5 << 2 | 2, 7 << 2 | 3], size=int(bad.sum()))           # no record; found only at the second try
            paths.append([int(c) for c in p])
    order = rng.permutation(len(paths))
    paths = [paths[int(k)] for k in order]
    tags = rng.integers(0, 4, size=len(paths)).astype(np.uint8)
    cls = run_plan(ctx, paths, tags, rec_len, rec_bits)
    seen = {int(c) for c in cls}
    assert {0, fr.WRITE, fr.WRITE | fr.PLAIN, fr.SELFGENE, fr.CYCLEGENE | fr.CYCLESCORE | fr.WRITE | fr.GENESCORE, fr.CYCLESCORE} <= seen, sorted(seen)


def test_the_edges_of_the_decision(ctx):
    #          0: 1 base, blast   1: 4 bases   2: 5 bases, blast   3: s09, 50   4: 949   5: 950   6: gene, 7   7: s07 only, 7   8: empty, gene
    rec_len = [1, 4, 5, 50, 949, 950, 7, 7, 0]
    rec_bits = [8, 0, 8, 6, 0, 0, 1, 2, 1]
    paths = [[0, 4 + 1], [0, 4, 0], [8 + 1, 4 + 1, 4, 4, 4, 4 + 1], [12, 16], [12, 20], [28, 20], [24], [28], [4], [12, 24], [32], [32, 4], []]
    for tag in range(4):
        cls = run_plan(ctx, paths, [tag] * len(paths), rec_len, rec_bits)
        if tag == 0:
            assert [int(c) for c in cls] == [0, fr.WRITE, 0, 0, fr.WRITE, 0, fr.WRITE, 0, 0, fr.WRITE | fr.GENESCORE, fr.WRITE, fr.WRITE, 0]
        if tag == 3:
            assert int(cls[6]) == fr.SELFGENE and int(cls[7]) == fr.SELFGENE and int(cls[8]) == fr.WRITE | fr.PLAIN and int(cls[3]) == fr.CYCLESCORE


def family(name):
    rng = np.random.default_rng(43)
    if name == "copies":
        one = [int(c) for c in rng.integers(0, 800, size=30)]
        paths = [list(one) for _ in range(4000)]
        paths[1234] = one[:-1] + [one[-1] ^ 1]
    else:
        base = [int(c) for c in rng.integers(0, 800, size=70)]
        variants = [base, base[:-1] + [base[-1] ^ 1], base[:-1] + [base[-1] + 4], base[:-1], base[:1], [c ^ 1 for c in base], base[1:], base + base[:1], [base[0] ^ 1],
                    [], base[:64], base[:65], base[:63] + [base[64], base[63]]]
        paths = [list(variants[int(k)]) for k in rng.integers(0, len(variants), size=1500)]
        paths += [[int(c) for c in rng.integers(0, 40, size=int(n))] for n in rng.integers(0, 3, size=1500)]
        paths = [paths[int(k)] for k in rng.permutation(len(paths))]
    classes = rng.choice([0, 1, 3, 4, 8, 16, 24, 57, 63], size=len(paths)).astype(np.uint8)
    return paths, classes


@pytest.mark.parametrize("name", ["copies", "near_equal"])
def test_first_of_equal(ctx, name):
    paths, classes = family(name)
    code = np.array([c for p in paths for c in p], np.int32)
    path_off = np.cumsum([0] + [len(p) for p in paths]).astype(np.int64)
    want = np.array(fr.first_of_equal([tuple(p) for p in paths], [int(c) for c in classes]), np.uint8)
    fp = capi.FilterPlan(ctx, code, path_off, [1])
    try:
        got = {bits: fp.first_of_equal(classes, bits) for bits in (64, 3, 0)}
    finally:
        fp.free()
    for bits, g in got.items():
        assert (g == want).all(), (bits, np.flatnonzero(g != want)[:10])
    assert (want & ~classes).max() == 0 and (name != "copies" or 0 < (want != 0).sum() <= 12)          # 4 000 equal paths: at most six firsts, and the odd one's
