"""csrc/depth.hip and csrc/depth_text.hip at the ABI: palace_depth_sum_covered, palace_depth_per_contig, palace_depth_text_create,
_emit and _windows against the exact restatement of tests/depth_text_cases.py (itself pinned by tests/test_host_depth_reference.py).
Bytes and integers only: every comparison is for equality.

Every case runs all five entry points and compares all their outputs; the cases aim at what the bamdepth executable never asks
for: tile and chunk-of-256-tiles borders, depths and positions at every step of their digit count, contigs shorter than one thread's
four positions, segments that do not count, emit ranges that begin and end anywhere, windows of any kind, call shapes of depth.hip.
Not covered: depths of 8 to 10 digits (10^7 and more segments on one position)."""
import numpy as np
import pytest

from palace_amd import capi
from tests import depth_text_cases as dtc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


_refs = {}


def ref_of(key, case):
    """the reference of a case, computed once per key"""
    if key not in _refs:
        _refs[key] = dtc.reference(case)
    return _refs[key]


def check_depth(ctx, case, ref, what=""):
    """the two entry points of depth.hip against the reference"""
    s, c = capi.depth_sum_covered(ctx, case.tlen, case.segs)
    assert (s, c) == (ref.sum, ref.lines), (what, "sum_covered")
    s, c, cs, cc = capi.depth_per_contig(ctx, case.tlen, (case.segs[:, 0], case.segs[:, 1], case.segs[:, 2]))
    assert (s, c) == (ref.sum, ref.lines), (what, "per_contig totals")
    assert np.array_equal(cs, ref.contig_sum), (what, "contig_sum", np.flatnonzero(cs != ref.contig_sum)[:8])
    assert np.array_equal(cc, ref.contig_covered), (what, "contig_covered", np.flatnonzero(cc != ref.contig_covered)[:8])


def first_difference(got, want):
    if len(got) != len(want):
        return ("length", len(got), len(want))
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    at = int(np.flatnonzero(a != b)[0])
    return (at, got[max(0, at - 30):at + 30], want[max(0, at - 30):at + 30])


def check_all(ctx, case, ref, what=""):
    """all outputs of all five entry points; -> the open DepthText (the caller closes it)"""
    check_depth(ctx, case, ref, what)
    dt = capi.DepthText(ctx, case.tlen, case.names, case.segs)
    try:
        assert (dt.text_bytes, dt.lines, dt.sum) == (len(ref.text), ref.lines, ref.sum), (what, "create")
        text, intact = dt.emit(0, dt.text_bytes)
        assert intact, (what, "emit wrote outside its range")
        assert text == ref.text, (what, "emit", first_difference(text, ref.text))
    except BaseException:
        dt.close()
        raise
    return dt


def run(ctx, case, ref, what=""):
    check_all(ctx, case, ref, what).close()


# ---- (a) tile geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["one_contig", "cut_at_1024"])
@pytest.mark.parametrize("total", dtc.GEOMETRY_TOTALS)
def test_tile_geometry(ctx, total, split):
    for pattern in dtc.GEOMETRY_PATTERNS:
        case = dtc.geometry_case(total, pattern, split)
        ref = dtc.reference(case)
        want = {"nothing": 0, "first": 1, "last": 1, "one_segment": total, "segment_per_position": total}.get(pattern)
        assert want is None or ref.lines == want
        run(ctx, case, ref, pattern)


# ---- (b) depth digit steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staggered", [False, True], ids=["stacked", "staggered"])
def test_depth_digit_steps(ctx, staggered):
    case = dtc.depth_digits_case(staggered)
    ref = ref_of(("digits", staggered), case)
    assert {len(l.split(b"\t")[2]) - 1 for l in ref.text_lines()} == set(range(1, 8))
    run(ctx, case, ref)


# ---- (c) position digit steps; emit's stride loop ---------------------------------------------------------------------------------------
def test_position_digit_steps_and_emit_stride(ctx):
    case = dtc.position_digits_case()
    ref = ref_of("positions", case)
    tiles = dtc.covered_tiles(ref)
    assert tiles[-1] - tiles[0] > dtc.EMIT_GRID                       # one emit launch has fewer workgroups than that: its loop runs
    assert {len(l.split(b"\t")[1]) for l in ref.text_lines()} == set(range(1, 9))
    run(ctx, case, ref)


# ---- (d), (e), (f) contig geometry, segments that do not count, any order ---------------------------------------------------------------
@pytest.mark.parametrize("with_ignored", [False, True], ids=["plain", "with_ignored"])
@pytest.mark.parametrize("with_long", [False, True], ids=["short", "with_1M_segment"])
def test_contig_geometry(ctx, with_long, with_ignored):
    case = dtc.contig_case(with_long, with_ignored)
    run(ctx, case, ref_of(("contigs", with_long, with_ignored), case))


@pytest.mark.parametrize("with_cut", [False, True], ids=["dropped_only", "with_the_cut_one"])
def test_ignored_segments_alone(ctx, with_cut):
    case = dtc.ignored_alone_case(with_cut)
    ref = dtc.reference(case)
    assert ref.lines == (3 if with_cut else 0)
    dt = check_all(ctx, case, ref)
    try:
        if not with_cut:                                              # nothing covered: all totals 0, per-contig arrays zeroed, emit(0, 0) taken
            assert (dt.text_bytes, dt.lines, dt.sum) == (0, 0, 0) and not ref.contig_sum.any() and not ref.contig_covered.any()
            assert dt.emit(0, 0) == (b"", True)
            tb, te, ln = dt.windows([0, -5, 3], [ref.total_len, 5, 1 << 40])
            assert not tb.any() and not te.any() and not ln.any()
    finally:
        dt.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_segment_order_does_not_matter(ctx, seed):
    ref = ref_of(("contigs", False, True), dtc.contig_case(False, True))
    case = dtc.contig_case(False, True, shuffle_seed=seed)
    assert not np.array_equal(case.segs, dtc.contig_case(False, True).segs)
    run(ctx, case, ref)


# ---- (g) emit ranges --------------------------------------------------------------------------------------------------------------------
def emit_cases():
    return {"contigs": dtc.contig_case(False, True), "sparse_tiles": dtc.sparse_tiles_case()}


@pytest.mark.parametrize("which", ["contigs", "sparse_tiles"])
def test_emit_ranges(ctx, which):
    case = emit_cases()[which]
    ref = ref_of(("contigs", False, True) if which == "contigs" else "sparse_tiles", case)
    if which == "sparse_tiles":
        assert (np.diff(dtc.covered_tiles(ref)) > 2).sum() >= 3
    ranges = dtc.emit_ranges(ref)
    assert len(ranges) > 15000
    dt = check_all(ctx, case, ref)
    try:
        for guard, some in ((16, ranges), (64, ranges[-1000:])):      # (the host allocates 16 spare bytes)
            for (a, b), (text, intact) in zip(some, dt.emit_many(some, guard)):
                assert intact, (a, b, "bytes outside [0, end - begin) written")
                assert text == ref.text[a:b], (a, b, first_difference(text, ref.text[a:b]))
        size = dt.text_bytes
        for a, b in [(5, 4), (size, size - 1), (0, size + 1), (size + 1, size + 2), (size - 3, size + 1)]:
            with pytest.raises(capi.PalaceError) as e:                # refused, and nothing launched: the buffer is as it was
                dt.emit(a, b)
            assert e.value.untouched, (a, b)
        assert dt.emit(dt.text_bytes, dt.text_bytes) == (b"", True)
    finally:
        dt.close()


# ---- (h) windows ------------------------------------------------------------------------------------------------------------------------
def windows_cases():
    """(d), and 257 tiles and 5 positions cut at 1024, most tiles empty: coverage on both sides of the borders at 1024, 2048, tile 100
    and tile 256 (where the tile scan starts its second chunk), and up to the last position"""
    T = dtc.TILE
    tlen = [T, 256 * T + 5]
    segs = [(0, 1000, 24), (1, 0, 3), (1, 700, 900), (1, 5000, 2500), (1, 99 * T - 1, 2), (1, 254 * T - 1, T + 2), (1, tlen[1] - 4, 4), (1, 255 * T + 1, 1)]
    return {"contigs": dtc.contig_case(False, True), "257_tiles": dtc.make_case(tlen, [b"left", b"right_of_1024"], segs)}


@pytest.mark.parametrize("which", ["contigs", "257_tiles"])
def test_windows(ctx, which):
    case = windows_cases()[which]
    ref = ref_of(("contigs", False, True) if which == "contigs" else "257_tiles", case)
    special, rnd = dtc.window_ranges(ref, 1001)
    assert len(special) > 40
    dt = check_all(ctx, case, ref)

    def ask(r):
        got, want = dt.windows(r[:, 0], r[:, 1]), ref.windows_reference(r[:, 0], r[:, 1])
        for g, w, name in zip(got, want, ("text_beg", "text_end", "lines")):
            bad = np.flatnonzero(g != w)
            assert len(bad) == 0, (name, len(r), r[bad[:4]].tolist(), g[bad[:4]].tolist(), w[bad[:4]].tolist())

    try:
        for n in (1, 3, 5):                                           # every special range in calls of n windows
            for k in range(0, len(special), n):
                ask(np.concatenate([special, special])[k:k + n])
        both = np.concatenate([special, rnd])
        ask(both[:1001])
        ask(both[-1001:])
    finally:
        dt.close()


# ---- (i) call shapes of depth.hip -------------------------------------------------------------------------------------------------------
def test_no_targets(ctx):
    for segs in ([], [(0, 0, 5), (-1, 3, 2)]):
        case = dtc.make_case([], [], segs)
        ref = dtc.reference(case)
        assert (ref.total_len, ref.lines, ref.sum) == (0, 0, 0)
        dt = check_all(ctx, case, ref)
        try:
            assert [x.tolist() for x in dt.windows([0, -1], [0, 5])] == [[0, 0]] * 3
        finally:
            dt.close()


def test_no_segments(ctx):
    case = dtc.make_case([5, 0, 2000], [b"a", b"b", b"c"], [])
    ref = dtc.reference(case)
    s, c, cs, cc = capi.depth_per_contig(ctx, case.tlen, case.segs)
    assert (s, c, cs.tolist(), cc.tolist()) == (0, 0, [0, 0, 0], [0, 0, 0])       # from 0xA5A5... to zero
    run(ctx, case, ref)


@pytest.mark.parametrize("n_segs", [1, 63, 64, 65, 255, 257])
def test_segment_counts_off_the_wave(ctx, n_segs):
    rng = np.random.default_rng(n_segs)
    tlen = [300, 1, 0, 4000, 77]
    tid = rng.integers(0, 5, size=n_segs)
    tid[0] = 3                                                        # (one segment at least on a contig that is not empty)
    pos = (rng.random(n_segs) * np.asarray(tlen)[tid]).astype(np.int64)
    case = dtc.make_case(tlen, [b"n%d" % t for t in range(5)], np.stack([tid, pos, rng.integers(1, 200, size=n_segs)], axis=1))
    ref = dtc.reference(case)
    assert ref.sum > 0
    run(ctx, case, ref)


def test_workspace_is_cleared_between_calls(ctx):
    """10 000 001 positions all covered, then on the same context 100 positions with one covered: a bit left in the bitmap shows"""
    big = dtc.make_case([7, dtc.LONG_CONTIG], [b"s", b"l"], [(1, 0, dtc.LONG_CONTIG), (0, 0, 7)])
    s, c, cs, cc = capi.depth_per_contig(ctx, big.tlen, big.segs)
    assert (s, c, cs.tolist(), cc.tolist()) == (dtc.LONG_CONTIG + 7, dtc.LONG_CONTIG + 7, [7, dtc.LONG_CONTIG], [7, dtc.LONG_CONTIG])
    assert capi.depth_sum_covered(ctx, big.tlen, big.segs) == (dtc.LONG_CONTIG + 7, dtc.LONG_CONTIG + 7)
    small = dtc.make_case([100], [b"small"], [(0, 41, 1)])
    assert capi.depth_sum_covered(ctx, small.tlen, small.segs) == (1, 1)
    s, c, cs, cc = capi.depth_per_contig(ctx, small.tlen, small.segs)
    assert (s, c, cs.tolist(), cc.tolist()) == (1, 1, [1], [1])
    run(ctx, small, dtc.reference(small))
