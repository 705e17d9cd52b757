"""palace_path_borders, palace_path_tandems, palace_paths_length_relation and palace_paths_base_set_in (csrc/path_dedup.hip) at the C ABI
against the brute force of tests/corrected_dup_cases.py.  Exact: every result is an integer.

Borders and tandems: random paths over 2 and over 5 tokens at every length where a wave (64), a workgroup's chunk (256) or a second
chunk begins or ends, planted periods 1, 64, 65 and n // 2, runs one short of a copy, exactly a copy and one short of two, a run
that ends on the path's last token, a path of 257 equal tokens, and 1, 2 and 300 paths a call with empty paths among them.  The count
call and the fill call must agree, and a cap one short is refused.
Relation: 1, 2, 64, 65 and 257 paths, the ratio at exactly 9/10 and at 8999/10000, equal sums, a repeated length, and a sum at the
refusal bound 2^49 and one below it.  Base sets: permuted lists with repeats, a strict subset, a superset, no cycles at all --
each at hash_bits 64, 2 and 0, where nearly every path collides."""
import numpy as np
import pytest

from palace_amd import capi
from tests import corrected_dup_cases as cd

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def check_borders(ctx, paths):
    vals, off = cd.flatten(paths)
    pd = capi.PathDedup(ctx, vals, off)
    try:
        got = pd.borders()
    finally:
        pd.free()
    want = np.array([cd.border(p) for p in paths], np.int32)
    assert (got == want).all(), np.flatnonzero(got != want)[:10]
    return want


def check_tandems(ctx, paths, brute=cd.tandem_candidates_np):
    vals, off = cd.flatten(paths)
    pd = capi.PathDedup(ctx, vals, off)
    try:
        count, off_count, off_fill, cand, intact = pd.tandems()
        if count:
            with pytest.raises(capi.PalaceError, match="cap"):
                pd.tandems(cap=count - 1)
    finally:
        pd.free()
    want = [np.asarray(brute(p), np.int32).reshape(-1, 3) for p in paths]
    want_off = np.cumsum([0] + [len(w) for w in want])
    assert count == want_off[-1] and intact
    assert (off_count == want_off).all() and (off_fill == want_off).all()
    assert (cand == np.concatenate(want)).all() if count else True
    return want


def random_paths(alphabet, seed):
    rng = np.random.default_rng(seed)
    return [[int(t) for t in rng.integers(0, alphabet, size=n)] for n in LENGTHS]


@pytest.mark.parametrize("alphabet", [2, 5])
def test_borders_random(ctx, alphabet):
    want = check_borders(ctx, random_paths(alphabet, 100 + alphabet))
    assert (want > 0).any()


def test_borders_planted(ctx):
    rng = np.random.default_rng(7)
    u = [int(t) for t in rng.integers(0, 1000, size=700)]
    paths = [[3] * 257, [3] * 256, u[:200] + [1001, 1002] + u[:200], u[:65] + u[:65], u[:64] + [1001] + u[:64], u[:300] + u[:299] + [1001],
             u[:1] + u[:1], u[:2] + u[1:2] + [1001], [], u[:700] + u[:700], [1001] + u[:100] + u[:100]]
    want = check_borders(ctx, paths)
    assert [int(x) for x in want] == [128, 128, 200, 65, 64, 0, 1, 0, 0, 700, 0]


@pytest.mark.parametrize("alphabet", [2, 5])
def test_tandems_random(ctx, alphabet):
    want = check_tandems(ctx, random_paths(alphabet, 200 + alphabet))
    assert sum(len(w) for w in want) > 500


def planted(r, k, lead=1):
    """lead distinct tokens, a unit of r distinct tokens, its first k tokens again, one closing token: R(r, lead) = k"""
    u = list(range(10, 10 + r))
    return list(range(5000, 5000 + lead)) + u + [u[q % r] for q in range(k)] + [9999]


def test_tandems_planted(ctx):
    paths = [[3] * 257]
    for r in (1, 64, 65, 70, 300):
        paths += [planted(r, r - 1), planted(r, r), planted(r, 2 * r - 1), planted(r, 2 * r), planted(r, r, lead=255)]
    u = list(range(100, 165))
    paths += [u + u, u[:64] + u[:64], [7] + u + u, [7, 8] + u[:64] + u[:64] + u[:64], u[:3] + [1, 2] * 100, u[:1] * 2, u[:2] * 2]      # periods n // 2; runs that end on the last token
    want = check_tandems(ctx, paths)
    assert len(want[0]) == sum(257 - 2 * r + 1 for r in range(1, 129))                      # equal tokens: every (r, s)
    for k, r in enumerate((1, 64, 65, 70, 300)):
        short, exact, almost, two, late = (want[1 + 5 * k + e] for e in range(5))
        assert not any(row[0] == r for row in short)
        assert [tuple(row) for row in exact if row[0] == r] == [(r, 1, 2)]
        assert {tuple(row) for row in almost if row[0] == r} == {(r, 1 + d, 2) for d in range(r)}
        assert (r, 1, 3) in {tuple(row) for row in two}
        assert [tuple(row) for row in late if row[0] == r] == [(r, 255, 2)]
    assert [tuple(row) for row in want[26]] == [(65, 0, 2)] and [tuple(row) for row in want[28]] == [(65, 1, 2)]


@pytest.mark.parametrize("n_paths", [1, 2, 300])
def test_tandems_many_paths(ctx, n_paths):
    rng = np.random.default_rng(n_paths)
    paths = []
    for k in range(n_paths):
        n = 0 if k % 3 == 1 else int(rng.integers(1, 90))
        paths.append([int(t) for t in rng.integers(0, 2, size=n)])
    if n_paths == 1:
        paths = [[int(t) for t in rng.integers(0, 2, size=77)]]
    check_tandems(ctx, paths, brute=cd.tandem_candidates)
    check_borders(ctx, paths)
    check_tandems(ctx, [[]] * n_paths)
    check_borders(ctx, [[]] * n_paths)


def check_relation(ctx, paths):
    vals, off = cd.flatten(paths, np.int64)
    pd = capi.PathDedup(ctx, vals, off, np.int64)
    try:
        got, intact = pd.length_relation()
    finally:
        pd.free()
    want = cd.length_relation(paths)
    assert intact and (got == want).all(), np.argwhere(got != want)[:10]
    return want


@pytest.mark.parametrize("n_paths", [1, 2, 64, 65, 257])
def test_relation_random(ctx, n_paths):
    rng = np.random.default_rng(300 + n_paths)
    pool = [int(x) for x in rng.integers(1, 5000, size=40)] + [100000, 100000, 7, 7]          # (lengths that two bases share)
    paths = []
    for k in range(n_paths):
        if k % 4 == 3:                                                                      # a relative of an earlier path: more, fewer or the same lengths
            p = list(paths[int(rng.integers(0, k))])
            p = p[:max(1, len(p) - int(rng.integers(0, 2)))] + [pool[int(rng.integers(0, 44))] for _ in range(int(rng.integers(0, 2)))]
            paths.append([p[int(q)] for q in rng.permutation(len(p))])
        else:
            paths.append([pool[int(q)] for q in rng.integers(0, 44, size=int(rng.integers(1, 70)))])      # (repeats inside a path)
    want = check_relation(ctx, paths)
    if n_paths >= 64:
        assert {0, 1, 2} <= {int(c) for c in want[np.triu_indices(n_paths, 1)]}


def test_relation_edges(ctx):
    paths = [[9, 1], [9, 100], [8999, 1001], [8999, 50000], [5, 5, 6], [6, 5], [6, 5, 5, 5], [1 << 28, 9 << 28], [9 << 28, 1 << 29, 3],
             [900000000000 // 300, 1], [], [4, 4, 4, 4]]
    want = check_relation(ctx, paths)
    assert want[0, 1] == cd.REL_I_LOSES                      # 9/10 of S(0) exactly, S(0) < S(1)
    assert want[2, 3] == cd.REL_NONE                         # 8999/10000
    assert want[4, 5] == cd.REL_I_LOSES and want[4, 6] == cd.REL_I_LOSES      # equal sums: i loses; a repeated length counts once
    assert want[7, 8] == cd.REL_I_LOSES and want[1, 0 + 2] == cd.REL_NONE
    assert want[0, 10] == cd.REL_J_LOSES                     # an empty path
    big = [(1 << 32) - 1 - k for k in range(1 << 17)]        # 2^17 distinct lengths just below 2^32 ...
    rest = (1 << 49) - 1 - sum(big)
    fill = [rest // 3 - 1, rest // 3, rest - 2 * (rest // 3) + 1]
    assert sum(big + fill) == (1 << 49) - 1 and len(set(big + fill)) == len(big) + 3 and max(fill) < min(big)
    tenth = [v for v in big[:1 << 13]]                       # ... and a path of some of them
    want = check_relation(ctx, [big + fill + fill[:1], tenth, big[:-1] + fill])              # a sum of 2^49 - 1 is taken
    assert want[0, 1] == cd.REL_J_LOSES and want[0, 2] == cd.REL_J_LOSES and want[1, 2] == cd.REL_I_LOSES
    vals, off = cd.flatten([big + fill[:2] + [fill[2] + 1], [5]], np.int64)                  # 2^49 is refused
    pd = capi.PathDedup(ctx, vals, off, np.int64)
    try:
        with pytest.raises(capi.PalaceError, match="2\\^49"):
            pd.length_relation()
    finally:
        pd.free()
    vals, off = cd.flatten([[1 << 32]], np.int64)                                           # a length that is no 32-bit number
    pd = capi.PathDedup(ctx, vals, off, np.int64)
    try:
        with pytest.raises(capi.PalaceError, match="token 0"):
            pd.length_relation()
    finally:
        pd.free()


def check_base_sets(ctx, paths, n_cycles):
    vals, off = cd.flatten(paths)
    pd = capi.PathDedup(ctx, vals, off)
    try:
        got = {bits: pd.base_set_in(n_cycles, bits) for bits in (64, 2, 0)}
    finally:
        pd.free()
    want = cd.base_set_in(paths, n_cycles)
    for bits, g in got.items():
        assert (g == want).all(), (bits, np.flatnonzero(g != want)[:10])
    return want


def test_base_sets(ctx):
    rng = np.random.default_rng(11)
    cycles = [[int(b) for b in rng.integers(0, 50, size=int(n))] for n in rng.integers(1, 80, size=70)] + [[], [4, 4, 4], [1 << 30, 0]]
    finals = []
    for c in cycles[:40]:
        s = sorted(set(c))
        perm = [s[int(q)] for q in rng.permutation(len(s))]
        finals += [perm + perm[:3], s[1:] if len(s) > 1 else [60], s + [51], perm[::-1] * 2]      # permuted with repeats; a strict subset; a superset
    finals += [[], [4], [0, 1 << 30, 0], [1 << 30], [int(b) for b in rng.integers(0, 50, size=300)]]
    want = check_base_sets(ctx, cycles + finals, len(cycles))
    assert want[:len(cycles)].sum() == 0 and 80 <= want.sum() < len(finals)
    assert list(want[-5:-1]) == [1, 1, 1, 0]
    assert check_base_sets(ctx, finals, 0).sum() == 0                                        # no cycles at all
    assert list(check_base_sets(ctx, [[1, 2], [2, 1, 1]], 1)) == [0, 1]
    assert list(check_base_sets(ctx, [[1, 2]], 1)) == [0]
