"""palace_blast_groups (csrc/filter_result.hip) at the C ABI against the restatement of tests/filter_result_cases.py: a table of some
3 000 lines and 30 tiles of PALACE_SAM_TILE with groups of 1, 2, 65 and several hundred lines, lines across tile borders, names longer
than a wavefront, the first-line rule both ways, a last line without LF, one-line and empty tables, identities at the cut and one
unit in the last place either side with 0, 3 and 6 decimals, group sums at, above and below the ratio -- and every fault code planted
at two lines, of which the smaller must be reported."""
import numpy as np
import pytest

from palace_amd import capi
from tests import filter_result_cases as fr

pytestmark = pytest.mark.gpu

TILE = 4096
LONG = b"contig_with_a_name_longer_than_one_wavefront_" + b"x" * 90 + b"_length_100"
RECORDS = [(b"r100_%d" % k, 100) for k in range(40)] + [(b"r10_%d" % k, 10) for k in range(6)] + [(LONG, 100), (LONG[:-1] + b"1", 100), (b"hollow", 0), (b"big", 45000),
                                                                                                  (b"one", 1)]
PAD = b"\t0\t0\t1\t100\t1\t100\t1e-20\t180.5"


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


@pytest.fixture(scope="module")
def fasta(ctx):
    text = b"".join(b">" + name + b" x\n" + (b"ACGTN" * (n // 5 + 1))[:n] + (b"\n" if n else b"") for name, n in RECORDS)
    f = capi.PathFasta(ctx, text)
    assert not f.duplicates().any() and [int(r[3]) for r in f.recs] == [n for _, n in RECORDS]
    return f


LENGTHS = dict(RECORDS)


def spell(value, k):
    digits = b"%0*d" % (k + 1, value)
    return digits if k == 0 else digits[:-k] + b"." + digits[-k:]


def table(ratio, first_passes, final_lf=True):
    """the lines of the good table, in groups; every probe has a query of its own, so its flag says what its lines added"""
    cuts = fr.identity_cuts(ratio * 100)
    rows = [(b"one", b"S", b"99.9" if first_passes else b"1.5", 1)]                      # the first line: inside its group
    q = iter(b"r100_%d" % k for k in range(40))
    for k in (0, 3, 6):                                                                 # 70 by the group's first line, 6 more iff the identity passes
        for value in (cuts[k] - 1, cuts[k], cuts[k] + 1):
            name = next(q)
            rows += [(name, b"S", b"0", 70), (name, b"S", spell(value, k), 6)]
    for total in (74, 75, 76, 69, 70, 71):                                              # sums at, above and below 0.75 and 0.7 of 100, over three lines
        name = next(q)
        rows += [(name, b"T", b"3.25", total - 20), (name, b"T", b"100", 15), (name, b"T", b"0.5", 1000), (name, b"T", b"100.000000", 5)]
    for k, total in enumerate((6, 7, 8)):                                               # 7 / 10
        rows.append((b"r10_%d" % k, b"S", b"50", total))
    name = next(q)
    rows += [(name, b"S1", b"100", 40), (name, b"S2", b"100", 40), (name, b"S1", b"100", 76)]      # one query, its subjects in turn: three groups
    rows += [(LONG, b"S", b"100", 30), (LONG, b"S", b"100", 45), (LONG[:-1] + b"1", b"S", b"100", 10), (LONG[:-1] + b"1", b"S" * 80, b"100", 76)]
    rows += [(next(q), b"S", b"100", 1)] * 65                                            # 65 lines: 1 + 64 when the first counts
    rows += [(b"big", b"S", b"100" if k % 3 else b"12.5", 17) for k in range(2900)]      # several hundred lines: many tiles, many workgroups
    rows += [(next(q), b"Z", b"100", 2)] * 2 + [(b"r10_5", b"Z", b"0", 8)]
    lines = [b"%s\t%s\t%s\t%d" % r + PAD[:len(PAD) - (k % 7)] for k, r in enumerate(rows)]
    return lines, b"\n".join(lines) + (b"\n" if final_lf else b"")


def check(ctx, fasta, text, ratio):
    got = capi.blast_groups(ctx, fasta, text, ratio)
    lines, groups, segs, bad_line, bad_code = fr.blast_groups(text, LENGTHS, ratio)
    assert got["intact"]
    assert (got["lines"], got["groups"], got["err_line"], got["err_code"]) == (lines, groups, bad_line, bad_code)
    want = np.array([name in segs for name, _ in RECORDS], np.uint8)
    assert (got["seg"] == want).all(), [RECORDS[k][0] for k in np.flatnonzero(got["seg"] != want)]
    assert got["flagged"] == len(segs)
    return got, segs


@pytest.mark.parametrize("ratio", [0.75, 0.7])
@pytest.mark.parametrize("first_passes", [False, True])
def test_the_large_table(ctx, fasta, ratio, first_passes):
    lines, text = table(ratio, first_passes, final_lf=first_passes)
    assert 2900 < len(lines) < 3300 and 110_000 < len(text) < 200_000
    starts = np.cumsum([0] + [len(v) + 1 for v in lines])
    assert sum(a // TILE != (b - 2) // TILE for a, b in zip(starts, starts[1:])) > 20   # lines across tile borders
    got, segs = check(ctx, fasta, text, ratio)
    assert (b"one" in segs) == first_passes and (b"big" in segs) == (ratio == 0.7) and b"r10_5" in segs            # big: 32878 / 45000
    probes = [b"r100_%d" % k in segs for k in range(9)]
    assert probes == [False, True, True] * 3                                            # below the cut, at it, above it; 0, 3 and 6 decimals
    assert [b"r100_%d" % k in segs for k in range(9, 15)] == ([False, False, True, False, False, False] if ratio == 0.75 else [True, True, True, False, False, True])
    assert [b"r10_%d" % k in segs for k in range(3)] == [False, False, True]            # 7 / 10 is not above 0.7
    assert b"r100_15" in segs and (LONG in segs) == (ratio == 0.7) and LONG[:-1] + b"1" in segs


def test_small_tables(ctx, fasta):
    for text in (b"", b"one\tS\t100\t1", b"one\tS\t100\t1\n", b"one\tS\t10\t1\n", b"r10_0\tS\t0\t8\nr10_0\tS\t0\t8\n", b"r10_0\tS\t0\t8\nr10_0\tT\t0\t8\n"):
        got, segs = check(ctx, fasta, text, 0.75)
    assert segs == {b"r10_0"} and got["groups"] == 2


FAULTS = {fr.E_COLUMNS: b"one\tS\t100", fr.E_NAME: b"\tS\t100\t1", fr.E_IDENTITY: b"one\tS\t100.\t1", fr.E_LENGTH: b"one\tS\t100\t12345678901",
          fr.E_QUERY: b"nobody\tS\t100\t1", fr.E_QEMPTY: b"hollow\tS\t100\t1"}


@pytest.mark.parametrize("code", sorted(FAULTS))
def test_every_fault_at_two_lines_reports_the_smaller(ctx, fasta, code):
    lines, _ = table(0.75, True)
    first, second = {1: (1, 2), 2: (2, len(lines)), 3: (1500, 1501), 4: (len(lines) - 1, len(lines)), 5: (40, 2999), 6: (700, 701)}[code]
    bad = list(lines)
    bad[first - 1] = bad[second - 1] = FAULTS[code]
    got, _ = check(ctx, fasta, b"\n".join(bad) + b"\n", 0.75)
    assert (got["err_line"], got["err_code"]) == (first, code) and not got["seg"].any()
    other = list(lines)                                                                  # another fault in front of it wins
    other[second - 1] = FAULTS[code]
    other[first - 1] = FAULTS[fr.E_COLUMNS if code != fr.E_COLUMNS else fr.E_NAME]
    got, _ = check(ctx, fasta, b"\n".join(other), 0.75)
    assert (got["err_line"], got["err_code"]) == (first, fr.E_COLUMNS if code != fr.E_COLUMNS else fr.E_NAME)
