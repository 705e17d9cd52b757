"""The ABI chain behind faidx's fetch (csrc/faidx.hip): palace_faidx_resolve -> palace_faidx_plan -> palace_faidx_write over an indexed
FASTA with its name table, byte for byte against the Python restatement of tests/faidx_cases.py (parity with `samtools faidx` is
UNPINNED: samtools is absent; tests/test_host_faidx_rules.py pins the restatement to a hand-typed catalogue).

Output offsets beyond 2^31 are NOT tested: such a text needs gigabytes of FASTA on the device and seconds per case.  All offsets of
the kernels are 64-bit; that is read from the code, not measured here."""
import numpy as np
import pytest

from palace_amd import capi
from tests import faidx_cases as fx
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu

LINE_LENS = (1, 15, 16, 17, 60, 61, 1000)
HEADER_LENS = (1, 14, 15, 16, 17)
TILE = capi.FASTA_TILE_BYTES


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def same(got: bytes, want: bytes):
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((len(got), len(want), at, got[max(0, at - 20):at + 20], want[max(0, at - 20):at + 20]))


def headers_for(n_regions: int):
    """headers of the caller's own, of the lengths at which a lane's 16 bytes begin and end"""
    return [(b"h%d_" % i + b"x" * 20)[:HEADER_LENS[i % len(HEADER_LENS)]] for i in range(n_regions)]


def model(text: bytes, regions):
    recs, code, _ = pc.fasta_index(text)
    assert code == pc.OK
    first_of = pc.first_records(recs)
    return recs, [fx.resolve(r, recs, first_of) for r in regions]


def resolved_on_device(fa, text, regions):
    recs, want = model(text, regions)
    got, d_regions = fa.resolve_regions(regions)
    assert [(int(g["rec"]), int(g["beg"]), int(g["len"])) for g in got] == want
    return recs, want, d_regions


def check_whole_text(fa, text, recs, want, d_regions, headers, n, reverse):
    off, total, first, planned = fa.plan(d_regions, len(want), headers, n, True)
    want_off = fx.plan(want, [len(h) for h in headers], n)
    assert list(off) == want_off and total == want_off[-1]
    assert first == next((i for i, w in enumerate(want) if w[0] < 0), -1)
    pieces, intact = fa.write(d_regions, len(want), planned, n, reverse, [(0, total)])
    assert intact, "bytes outside the window were written"
    same(pieces[0], fx.abi_text(text, recs, want, headers, n, reverse))
    return total, planned


def grid_fasta(rng, line_bases: int, eol: bytes, final_eol: bool):
    """records of 0 bases (no sequence line), 1, a line less one, a line, a line and one, several lines and a part, and one long
    enough for two output lines of 1000"""
    lengths = [0, 1, max(line_bases - 1, 1), line_bases, line_bases + 1, 5 * line_bases + 3, 2100, 37]
    return pc.fasta_text([(b"r%d" % i, pc.random_seq(rng, n)) for i, n in enumerate(lengths)], line_bases, eol, final_eol)


def grid_regions(n: int):
    """a whole record, mid-line starts and ends, lengths 0, 1, n and 2n, a failed and a 0-base region between written ones"""
    return [b"r6", b"r5:2-", b"r6:%d-%d" % (3, 2 + n), b"nowhere:1-5", b"r6:%d-%d" % (11, 10 + 2 * n), b"r0", b"r1", b"r6:5000", b"r6:77-77",
            b"r6:-%d" % n, b"r2", b"r3", b"r4", b"r6:x", b"r7:30-", b"r5:4-9", b"r7"]


@pytest.mark.parametrize("eol,final_eol", [(b"\n", True), (b"\r\n", True), (b"\n", False)], ids=["lf", "crlf", "no_final_lf"])
@pytest.mark.parametrize("line_bases", [1, 7, 15, 16, 17, 60, 61, 70])
def test_source_grids_line_lengths_and_strands(ctx, line_bases, eol, final_eol):
    rng = np.random.default_rng(100 * line_bases + len(eol) + 2 * final_eol)
    text = grid_fasta(rng, line_bases, eol, final_eol)
    fa = capi.Faidx(ctx, text)
    try:
        for n in LINE_LENS:
            regions = grid_regions(n)
            recs, want, d_regions = resolved_on_device(fa, text, regions)
            assert sum(w[0] < 0 for w in want) == 2 and sum(w[0] >= 0 and w[2] == 0 for w in want) == 2
            assert {1, n, 2 * n} <= {w[2] for w in want}
            for reverse in (False, True):
                check_whole_text(fa, text, recs, want, d_regions, headers_for(len(regions)), n, reverse)
    finally:
        fa.close()


@pytest.fixture(scope="module")
def tiles(ctx):
    """more than two tiles of output from 600 tiny regions, and one record that spans several tiles"""
    rng = np.random.default_rng(7)
    text = pc.fasta_text([(b"t%d" % i, pc.random_seq(rng, 1 + i % 9)) for i in range(600)] + [(b"long", pc.random_seq(rng, 3 * TILE + 123))], 70)
    regions = [b"t%d" % i if i % 3 else b"t%d:2-3" % i for i in range(600)] + [b"long", b"gone", b"t5:99", b"long:100-4300"]
    fa = capi.Faidx(ctx, text)
    recs, want, d_regions = resolved_on_device(fa, text, regions)
    headers = headers_for(len(regions))
    out = {}
    for reverse in (False, True):
        total, planned = check_whole_text(fa, text, recs, want, d_regions, headers, 61, reverse)
        out[reverse] = (planned, fx.abi_text(text, recs, want, headers, 61, reverse))
    assert fx.plan(want, [len(h) for h in headers], 61)[600] > 2 * TILE and total > 5 * TILE
    yield fa, d_regions, len(regions), out
    fa.close()


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
@pytest.mark.parametrize("win", [1, 16, 17, 4096, 4097])
def test_windows_of_every_size_give_the_same_text(tiles, win, reverse):
    fa, d_regions, n_regions, out = tiles
    planned, want = out[reverse]
    total = len(want) if win > 1 else 3000                                       # (windows of one byte: the text's first 3000)
    bounds = [(lo, min(lo + win, total)) for lo in range(0, total, win)]
    pieces, intact = fa.write(d_regions, n_regions, planned, 61, reverse, bounds)
    assert intact, "bytes outside a window were written"
    same(b"".join(pieces), want[:total])


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reverse"])
def test_every_lo_and_every_hi_of_a_small_text(ctx, reverse):
    text = b">a\nACGTNRYacgt\nKMBVDHkmbvd\nAC\n>b\n>c\nGATTACAGATTACAGATTACAGATTACAGATTACA\n"
    regions = [b"a", b"b", b"zz", b"c:3-30", b"a:100", b"c:35", b"a:12-13"]
    fa = capi.Faidx(ctx, text)
    try:
        recs, want, d_regions = resolved_on_device(fa, text, regions)
        headers = [b"a", b"fourteen_bytes", b"", b"c:3-30_16_bytes_", b"seventeen_bytes_h", b"fifteen_bytes_h", b"a:12-13"]
        total, planned = check_whole_text(fa, text, recs, want, d_regions, headers, 7, reverse)
        whole = fx.abi_text(text, recs, want, headers, 7, reverse)
        assert 100 < total <= 200 and {len(h) for h, w in zip(headers, want) if w[0] >= 0} == set(HEADER_LENS) | {7}
        bounds = [(lo, total) for lo in range(total + 1)] + [(0, hi) for hi in range(total + 1)]
        pieces, intact = fa.write(d_regions, len(regions), planned, 7, reverse, bounds)
        assert intact, "bytes outside a window were written"
        for (lo, hi), piece in zip(bounds, pieces):
            assert piece == whole[lo:hi], (lo, hi)
    finally:
        fa.close()


def test_no_regions(ctx):
    fa = capi.Faidx(ctx, b">a\nACGT\n")
    try:
        got, d_regions = fa.resolve_regions([])
        assert len(got) == 0
        off, total, first, planned = fa.plan(d_regions, 0, [], 60, True)
        assert (list(off), total, first) == ([0], 0, -1)
        pieces, intact = fa.write(d_regions, 0, planned, 60, False, [(0, 0)])
        assert intact and pieces == [b""]
    finally:
        fa.close()


def test_resolve_over_the_grammar_catalogue(ctx):
    regions = fx.GRAMMAR_REGIONS + [b"", b":", b"chr1:9999999999999999999-", b"chr1:-1234567890123456789"]
    fa = capi.Faidx(ctx, fx.CATALOGUE_FASTA)
    try:
        _, want, _ = resolved_on_device(fa, fx.CATALOGUE_FASTA, regions)
        assert want[regions.index(b"chr1:3-12")] == (0, 2, 10) and want[regions.index(b"a:b:2-3")] == (2, 0, 4) and want[regions.index(b"a:b:2-4")] == (1, 1, 3)
        assert all(want[regions.index(r)] == (-1, 0, 0) for r in (b"", b":", b"chr1:1234567890123456789", b"chr1:9999999999999999999-", b"chr1:5-4"))
        assert want[regions.index(b"chr1:123456789012345678")] == (0, 25, 0)
    finally:
        fa.close()


def test_resolve_over_many_names(ctx):
    rng = np.random.default_rng(11)
    text, names = fx.synthetic_assembly(rng, 3000, max_len=90)
    regions = []
    for i in rng.integers(0, len(names), size=5000):
        b, e = sorted(int(x) for x in rng.integers(0, 120, size=2))
        regions.append((names[i], names[i] + b":%d-%d" % (b, e), names[i] + b":%d" % b, names[i] + b"x", names[i] + b":-%d" % e)[int(rng.integers(0, 5))])
    fa = capi.Faidx(ctx, text)
    try:
        _, want, _ = resolved_on_device(fa, text, regions)
        assert sum(w[0] < 0 for w in want) > 500 and sum(w[0] >= 0 and w[2] == 0 for w in want) > 100
    finally:
        fa.close()


@pytest.mark.parametrize("n", [1, 16, 60])
def test_plan_offsets_and_the_first_failed_region(ctx, n):
    fa = capi.Faidx(ctx, b">a\nACGT\n")
    try:
        rng = np.random.default_rng(n)
        for n_regions, failed in ((1, []), (1, [0]), (5, [4]), (2500, [1700, 2047, 2048]), (2500, []), (1025, [1024])):
            resolved = [(-1, 0, 0) if i in failed else (0, int(rng.integers(0, 4)), int(rng.integers(0, 200))) for i in range(n_regions)]
            headers = headers_for(n_regions)
            d_regions = fa.upload_regions(resolved)
            want = fx.plan(resolved, [len(h) for h in headers], n)
            off, total, first, _ = fa.plan(d_regions, n_regions, headers, n, True)
            assert (list(off), total, first) == (want, want[-1], failed[0] if failed else -1)
            off, total, first, _ = fa.plan(d_regions, n_regions, headers, n, False)
            assert first == (failed[0] if failed else -1)
            assert (list(off), total) == (([0] * (n_regions + 1), 0) if failed else (want, want[-1]))
            d_regions.free()
    finally:
        fa.close()
