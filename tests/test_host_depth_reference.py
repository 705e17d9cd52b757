"""The reference of tests/depth_text_cases.py, which judges the depth kernels at the ABI (tests/test_gpu_depth_abi.py), pinned to two
statements that were there before it -- expected_depth_text of tests/test_host_depthgz.py and the hand-derived 150 bytes there -- and
to a text typed by hand.  Also: the case builders build what their names say."""
import numpy as np

from palace_amd import synth
from tests import depth_text_cases as dtc
from tests.test_host_depthgz import expected_depth_text


def segments_of(records):
    """the CIGAR walk of expected_depth_text, reduced to (tid, pos, len) per M / = / X operation; nothing cut"""
    segs = []
    for r in records:
        if r.flag & 0x704 or r.tid < 0 or r.pos < 0:
            continue
        p = r.pos
        for n, op in synth.parse_cigar(r.cigar):
            if op in (0, 7, 8):
                segs.append((r.tid, p, n))
                p += n
            elif op in (2, 3):
                p += n
    return segs


def same_as_expected(targets, records):
    lines, per_contig, total, nr = expected_depth_text(targets, records)
    ref = dtc.Reference([l for _, l in targets], [n.encode() for n, _ in targets], segments_of(records))
    assert ref.text == b"".join(lines) and ref.text_lines() == lines
    assert (ref.sum, ref.lines) == (total, nr)
    for t, (name, _) in enumerate(targets):
        mine = per_contig.get(name, [])
        assert int(ref.contig_covered[t]) == len(mine) and int(ref.contig_sum[t]) == sum(int(l.split(b"\t")[2]) for l in mine)
    return ref


def test_equals_expected_depth_text_on_a_random_case():
    rng = synth.rng_for(3)
    targets, _, recs, _ = synth.random_graph_case(rng, 60, 6000)
    for k in range(200):                      # skipped flags, deletions / skips / clips / insertions, reads over the contig end
        t = int(rng.integers(0, len(targets)))
        cig = ["20M5D30M", "10S40M", "25M3I25M2N20M", "30=5X15M", "50M"][k % 5]
        recs.append(synth.BamRecord(f"x{k}", [0, 0x400, 0x100, 0x200, 0x4, 0x800, 16][k % 7], t, int(rng.integers(0, targets[t][1])), 60, cig))
    ref = same_as_expected(targets, recs)
    assert ref.lines > 1000 and ref.sum > ref.lines


def test_equals_the_hand_derived_150_bytes():
    targets = [("c1", 100), ("c2", 20000)]
    recs = [synth.BamRecord("r1", 0, 0, 10, 60, "5M"), synth.BamRecord("r2", 0, 1, 16380, 60, "10M")]
    ref = same_as_expected(targets, recs)
    want = b"".join(b"c1\t%d\t1\n" % q for q in range(11, 16)) + b"".join(b"c2\t%d\t1\n" % q for q in range(16381, 16391))
    assert ref.text == want and len(want) == 150 and (ref.sum, ref.lines) == (15, 15)
    # the two 16 kb windows of c2 as that test derives them: [40, 84) with 4 lines, [84, 150) with 6
    tb, te, ln = ref.windows_reference([100, 100 + 16384], [100 + 16384, 100 + 20000])
    assert tb.tolist() == [40, 84] and te.tolist() == [84, 150] and ln.tolist() == [4, 6]


def test_equals_a_text_typed_by_hand():
    """a (4 bases), bb (3 bases).  (a, 2, 5) is cut at a's end: a:3 and a:4.  (bb, 0, 2) and (bb, 1, 1): bb:1 once, bb:2 twice.
    (bb, 3, 1) starts at bb's end and (2, 0, 1) names no contig: dropped."""
    ref = dtc.Reference([4, 3], [b"a", b"bb"], [(0, 2, 5), (1, 0, 2), (1, 1, 1), (1, 3, 1), (2, 0, 1)])
    assert ref.text == b"a\t3\t1\na\t4\t1\nbb\t1\t1\nbb\t2\t2\n"
    assert (ref.sum, ref.lines, ref.total_len) == (5, 4, 7)
    assert ref.contig_sum.tolist() == [2, 3] and ref.contig_covered.tolist() == [2, 2]
    assert ref.line_off.tolist() == [0, 6, 12, 19, 26] and ref.line_g.tolist() == [2, 3, 4, 5]
    tb, te, ln = ref.windows_reference([0, 3, 5, -3, 7, 6], [4, 100, 2, 3, 9, 6])
    assert tb.tolist() == [0, 6, 19, 0, 26, 26] and te.tolist() == [12, 26, 19, 6, 26, 26] and ln.tolist() == [2, 3, 0, 1, 0, 0]


def test_segment_rule_on_the_edges_of_int32():
    tlen = [0, 5, 1024, 0, 70]
    for t in (1, 2, 4):
        tid, a, b = dtc.kept_segments(tlen, dtc.ignored_segments(tlen, t))
        assert (tid.tolist(), a.tolist(), b.tolist()) == ([t], [tlen[t] - 1], [tlen[t]])
    assert dtc.reference(dtc.ignored_alone_case(False)).lines == 0
    ref = dtc.reference(dtc.ignored_alone_case(True))
    assert ref.text == b"five\t5\t1\ntile\t1024\t1\nseventy\t70\t1\n"


def test_builders_build_what_they_promise():
    ref = dtc.reference(dtc.position_digits_case())
    tiles = dtc.covered_tiles(ref)
    assert tiles[-1] - tiles[0] > dtc.EMIT_GRID and ref.lines == 16
    assert [int(l.split(b"\t")[1]) for l in ref.text_lines()[1:]] == [q for e in range(1, 8) for q in (10 ** e - 1, 10 ** e)] + [10_000_001]
    case = dtc.contig_case(with_ignored=True)
    base = np.concatenate([[0], np.cumsum(case.tlen)])
    empty = [t for t, l in enumerate(case.tlen) if l == 0]
    assert empty[0] == 0 and empty[-1] == len(case.tlen) - 1 and any(base[t] % dtc.TILE == 0 and base[t] > 0 for t in empty)
    assert len(set(case.names)) < len(case.names)
    ref = dtc.reference(case)
    assert 4000 < len(ref.text) < 40000 and ref.line_g[-1] == ref.total_len - 1
    assert dtc.reference(dtc.contig_case(shuffle_seed=1)).text == dtc.reference(dtc.contig_case()).text
    for staggered in (False, True):
        ref = dtc.reference(dtc.depth_digits_case(staggered))
        depths = {int(l.split(b"\t")[2]) for l in ref.text_lines()}
        assert set(dtc.DEPTH_STEPS) <= depths
        assert ref.sum == sum(40 * k - int((np.arange(k) % 7).sum()) if staggered else 35 * k for k in dtc.DEPTH_STEPS)
    tiles = dtc.covered_tiles(dtc.reference(dtc.sparse_tiles_case()))
    assert (np.diff(tiles) > 2).sum() >= 3
