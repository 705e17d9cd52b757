"""csrc/bam_index.hip at the ABI: palace_bai_records, palace_bai_chunks, palace_bai_linear and palace_bgzf_voffsets against the exact
restatement of tests/bai_cases.py (itself pinned by tests/test_host_bai_reference.py), on streams built here from record encodings
behind an odd-length stand-in header -- no BGZF involved.  Integers only: every comparison is for equality.

The cases aim at what the bamsort executable's tests never reach: status words met from several workgroups, more than one workgroup
of the strip kernels (4 096 records) and of the per-reference kernels (256 references), run keys with a reference bit above 16, more
runs than one sort tile and more than 1 024 blocks of the head scan, count-only and short-cap calls, calls without records or without
references, member tables with empty members and file offsets of 2^32 and more.  Every condition a case depends on is asserted on
the reference before the device is called.

Not observable here: the `done` clamp of bai_linear_kernel only saves atomics -- on a sorted stream a window written a second time
keeps its smaller, earlier offset -- so no output can tell whether it is there."""
import random

import numpy as np
import pytest

from palace_amd import capi
from tests import bai_cases as bai
from tests import bam_sort_cases as bc
from tests.test_host_bam_spec import record

pytestmark = pytest.mark.gpu

HEAD = bytes(range(101))                    # a stand-in for the header; its odd length puts the records at no alignment
STRIP, STRIP_GROUP = 16, 4096               # records a lane of the strip kernels folds, records one of their workgroups covers


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx() as c:
        yield c


def layout(recs):
    starts, sizes = bai.starts_and_sizes(recs, len(HEAD))
    return HEAD + b"".join(recs), starts, sizes


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = np.flatnonzero(got != want)
    assert len(differ) == 0, (what, len(differ), [(int(k), got[k].item(), want[k].item()) for k in differ[:8]])


def check_columns(got, col, what=""):
    """the five columns of palace_bai_records; of a record a .bai cannot hold only `unmapped` is specified"""
    good = ~col.bad
    for name, g, w in zip(("ref", "bin", "win_beg", "win_end"), got, (col.ref, col.bin, col.win_beg, col.win_end)):
        assert len(g) == len(w), (what, name)
        same(g[good], w[good], (what, name))
    same(got[4], col.unmapped, (what, "unmapped"))


def check_chunks(got, want, what=""):
    for name, g, w in zip(("chunk_ref", "chunk_bin", "chunk_beg", "chunk_end"), got, want):
        same(g, w, (what, name))


def check_linear(got, ln, what=""):
    n_intv, stat, lin_off, lin = got
    same(n_intv, ln.n_intv, (what, "n_intv"))
    same(stat[0], ln.n_mapped, (what, "records with flag 0x4 clear"))
    same(stat[1], ln.n_unmapped, (what, "records with flag 0x4 set"))
    same(stat[2][ln.used], ln.first[ln.used], (what, "first offset"))      # (undefined for a reference without records)
    same(stat[3][ln.used], ln.last[ln.used], (what, "last offset"))
    same(lin_off, ln.lin_off, (what, "lin_off"))
    same(lin, ln.lin, (what, "lin"))


def check_index(ctx, recs, n_ref, what=""):
    """records -> chunks -> linear as host/bai.hpp calls them, every output against the reference -> (the device's outputs, the
    reference's)"""
    stream, starts, sizes = layout(recs)
    col = bai.columns(recs, n_ref)
    assert col.status[:3] == (0, -1, -1), (what, col.status)
    want_runs = bai.runs(col.ref, col.bin, starts, sizes, n_ref)
    ln = bai.linear(col.ref, col.win_beg, col.win_end, col.unmapped, starts, sizes, n_ref)
    *cols, status = capi.bai_records(ctx, stream, starts, n_ref)
    assert status == col.status, (what, status, col.status)
    check_columns(cols, col, what)
    n_runs, *chunks = capi.bai_chunks(ctx, stream, starts, cols[0], cols[1], n_ref)
    assert n_runs == len(want_runs[0]), (what, n_runs)
    check_chunks(chunks, want_runs, what)
    lin = capi.bai_linear(ctx, stream, starts, cols[0], cols[2], cols[3], cols[4], n_ref)
    check_linear(lin, ln, what)
    return dict(status=status, chunks=chunks, linear=lin), dict(col=col, runs=want_runs, linear=ln, stream=stream)


# ---- the columns of hand-made records ------------------------------------------------------------------------------------------
N_REF_HAND = 7


def hand_records():
    """the good ones of tests/test_host_bam_index_rules.py's hand cases"""
    recs = [record("unplaced_with_pos", 4, -1, 777, 0, "", l_seq=5), record("reverse", 16, 1, 100, 60, "50M"), record("forward", 0, 1, 100, 60, "50M"),
            record("zero_m", 0, 1, 200, 60, "0M", l_seq=4), record("only_s_i", 0, 1, 300, 60, "5S7I"), record("unmapped_with_cigar", 4, 1, 400, 0, "30M"),
            record("no_ops", 0, 3, 16383, 0, "", l_seq=9), bc.cg_record("cg", 0, 2, 7, "10S" + "1M1D" * 40 + "50M5S"),
            record("fake_placeholder", 0, 2, 9, 30, [(50 << 4) | 4, (60 << 4) | 3], l_seq=50)]
    for shift in (14, 17, 20, 23, 26, 29):
        edge = 1 << shift
        recs += [record(f"on_{shift}", 0, 0, edge - 40, 0, "40M"), record(f"before_{shift}", 0, 0, edge - 41, 0, "40M")]
        if shift < 29:
            recs += [record(f"across_{shift}", 0, 0, edge - 39, 0, "40M"), record(f"at_{shift}", 0, 0, edge, 0, "1M")]
    return bc.sorted_records(recs, N_REF_HAND)


def test_columns_of_hand_made_records(ctx):
    recs = hand_records()
    col = bai.columns(recs, N_REF_HAND)
    names = [r[36:r.index(b"\0", 36)].decode() for r in recs]
    at = {n: k for k, n in enumerate(names)}
    assert col.status == (0, -1, -1, 1) and names[-1] == "unplaced_with_pos"
    assert (col.ref[-1], col.bin[-1], col.win_beg[-1], col.win_end[-1], col.unmapped[-1]) == (-1, 0, 0, 0, 1)
    assert col.bin[at["on_29"]] == 4681 + 32767 and col.win_end[at["on_29"]] == 32767 and col.bin[at["across_26"]] == 0 and col.bin[at["across_14"]] == 585
    assert [(col.win_beg[at[n]], col.win_end[at[n]]) for n in ("zero_m", "only_s_i", "unmapped_with_cigar", "no_ops")] == [(0, 0), (0, 0), (0, 0), (0, 0)]
    assert col.bin[at["no_ops"]] == 4681 and col.bin[at["cg"]] == col.bin[at["fake_placeholder"]] == 4681
    check_index(ctx, recs, N_REF_HAND, "hand")


# ---- the status words, met from several workgroups -------------------------------------------------------------------------------------
STATUS_TARGETS = [("a", 1 << 29), ("b", 5000), ("c", 300000), ("d", 70000), ("e", 40)]
N_TAIL = 200


def status_base():
    """2 900 sorted placed records and a tail of 200 without a contig: 13 workgroups of palace_bai_records"""
    rng = random.Random(4201)
    placed = bc.sorted_records(bc.random_records(rng, 2900, STATUS_TARGETS, unplaced=0.0), len(STATUS_TARGETS))
    tail = [record(f"u{k}", 4 | (16 if k >= N_TAIL // 2 else 0), -1, -1, 0, "", l_seq=k % 7) for k in range(N_TAIL)]
    return placed, tail


def bad_records_case():
    placed, tail = status_base()
    n_ref = len(STATUS_TARGETS)
    recs = placed + tail
    k0 = sum(1 for r in placed if bc.fields(r)["tid"] == 0)                 # behind reference 0's records: where its key sorts it
    past = record("past_the_scheme", 0, 0, (1 << 29) - 3, 0, "4M")           # end = 2^29 + 1; it has a key
    bad = [(k0, past), (1500, record("bad_tid", 0, n_ref, 5, 0, "5M")), (1501, record("bad_pos", 0, 2, -2, 0, "5M")), (2900, record("bad_tid_low", 0, -2, 5, 0, "5M"))]
    for k, r in bad:
        recs.insert(k, r)
    assert k0 >= 256 and len({k // 256 for k, _ in bad}) == 3 and all(recs[k] is r for k, r in bad)
    return recs, k0, n_ref


def test_bad_records_in_three_workgroups(ctx):
    recs, k0, n_ref = bad_records_case()
    col = bai.columns(recs, n_ref)
    assert col.status == (4, k0, -1, N_TAIL) and np.flatnonzero(col.bad).tolist() == [k0, 1500, 1501, 2900]
    stream, starts, _ = layout(recs)
    *cols, status = capi.bai_records(ctx, stream, starts, n_ref)
    assert status == col.status
    check_columns(cols, col, "bad records")


def unsorted_case():
    placed, tail = status_base()
    n_ref = len(STATUS_TARGETS)
    key = [bc.sort_key(r, n_ref) for r in placed]
    k1 = 1277                                                               # after the insertions below the first pair straddles two workgroups
    later = tuple(next(k for k in range(p, p + 100) if key[k] < key[k + 1]) for p in (1800, 2300, 2700))
    assert all(key[k] < key[k + 1] for k in (k1,) + later)
    recs = placed[:]
    for k in (k1,) + later:
        recs[k], recs[k + 1] = recs[k + 1], recs[k]
    recs += tail
    # two records without a key: alone among sorted neighbours, and right in front of the first swapped pair
    recs.insert(k1, record("bad_pos", 0, bc.fields(placed[k1])["tid"], -2, 0, "5M"))
    recs.insert(600, record("bad_tid_low", 0, -2, 5, 0, "5M"))
    first = k1 + 3
    assert (first - 1) // 256 != first // 256 and len({first // 256} | {(k + 3) // 256 for k in later}) == 4
    return recs, first, n_ref


def test_unsorted_pairs_in_several_workgroups(ctx):
    recs, first, n_ref = unsorted_case()
    col = bai.columns(recs, n_ref)
    assert col.status == (2, 600, first, N_TAIL), col.status
    stream, starts, _ = layout(recs)
    *cols, status = capi.bai_records(ctx, stream, starts, n_ref)
    assert status == col.status
    check_columns(cols, col, "unsorted")


def test_tail_of_unplaced_records_ends_in_a_partial_wave(ctx):
    placed, tail = status_base()
    recs = placed + tail
    assert len(recs) % 64 != 0 and (len(recs) - 1) // 64 - len(placed) // 64 + 1 >= 3
    got, want = check_index(ctx, recs, len(STATUS_TARGETS), "tail")
    assert got["status"] == (0, -1, -1, N_TAIL)
    assert want["runs"][0][-1] == -1 and (want["runs"][0] == -1).sum() == 1 and want["runs"][3][-1] == len(want["stream"])


# ---- many references -----------------------------------------------------------------------------------------------------------------
N_REF_MANY = 70000


def many_references_case():
    rng = random.Random(4304)
    recs, used = bai.many_reference_records(rng, N_REF_MANY, 2000, 100000, 37)
    recs = bc.sorted_records(recs, N_REF_MANY)
    ref = np.array([bc.fields(r)["tid"] for r in recs])
    n = len(recs)
    assert n > STRIP_GROUP                                                  # the strip kernels run in at least two workgroups
    assert any(len(set(ref[s:s + STRIP].tolist()) - {-1}) >= 3 for s in range(0, n, STRIP))
    assert any(ref[k - 1] == ref[k] >= 0 for k in range(STRIP_GROUP, n, STRIP_GROUP))   # a reference met by two workgroups
    assert max(used) >= 65536 and set(bai.FORCED_REFS) <= set(used)
    assert max(b - a for a, b in zip(used, used[1:])) >= 1000               # whole workgroups of the per-reference kernels without a record
    return recs


def test_many_references(ctx):
    recs = many_references_case()
    got, want = check_index(ctx, recs, N_REF_MANY, "many references")
    ln = want["linear"]
    assert int(ln.used.sum()) == 2009 and got["status"][3] == 37
    # the file's bytes from the device's arrays and from the reference's, with a made-up table of one member
    mu, mc = [0, len(want["stream"])], [0x1234, 0x1234 + 999]
    n_intv, stat, lin_off, lin = got["linear"]
    mine = bai.bai_bytes(N_REF_MANY, got["chunks"], n_intv, stat[0], stat[1], stat[2], stat[3], lin_off, lin, got["status"][3],
                         lambda u: capi.bgzf_voffsets(ctx, u, mu, mc))
    theirs = bai.bai_bytes(N_REF_MANY, want["runs"], ln.n_intv, ln.n_mapped, ln.n_unmapped, ln.first, ln.last, ln.lin_off, ln.lin, want["col"].status[3],
                           lambda u: bai.voffsets(u, mu, mc))
    assert len(mine) == len(theirs) and mine == theirs


# ---- the shapes of the linear index on one reference ---------------------------------------------------------------------------------
def one_reference_records(spanning):
    """about 5 000 records on one reference of 2^29 bases: nothing in front of window 5, 60 records that all start and end in window
    5, islands of records with untouched windows between them, spliced records over seven windows, and one last record in the last
    window; `spanning`: also a record from window 0 to the last one"""
    rng = random.Random(4400)
    win = 1 << 14
    recs = [record(f"same{k}", 0, 0, 5 * win + 10 * k, 60, "30M") for k in range(60)]
    for island in range(300):
        at = rng.randrange(8, 8000) * win
        for k in range(16):
            pos = at + rng.randrange(0, 3 * win)
            recs.append(record(f"i{island}_{k}", 16 * rng.randrange(2), 0, pos, 60, "50M100000N50M" if rng.random() < 0.06 else f"{rng.randrange(1, 150)}M"))
    recs.append(record("last", 0, 0, (1 << 29) - 100, 60, "100M"))
    if spanning:
        recs.append(record("whole", 0, 0, 5, 60, f"10M{(1 << 28) - 20}N{(1 << 28) - 5}N10M"))
    return bc.sorted_records(recs, 1)


@pytest.mark.parametrize("spanning", [False, True], ids=["gaps", "spanning"])
def test_linear_index_on_one_reference(ctx, spanning):
    recs = one_reference_records(spanning)
    col = bai.columns(recs, 1)
    wb, we = col.win_beg, col.win_end
    touched = np.zeros(1 << 15, bool)
    for a, b in zip(wb, we):
        touched[a:b + 1] = True
    assert 4800 < len(recs) < 5200 and (we - wb).max() >= (32767 if spanning else 6)
    assert any((wb[s:s + STRIP] == wb[s]).all() and (we[s:s + STRIP] == wb[s]).all() for s in range(0, len(recs) - STRIP, STRIP))   # a strip with nothing new
    assert we.max() == 32767 and (we == 32767).sum() == (2 if spanning else 1)
    if spanning:
        assert touched.all() and (wb[0], we[0]) == (0, 32767)
    else:
        assert not touched[:5].any() and touched[5] and we[-1] == 32767 and np.sort(we)[-2] < 9000     # the last record alone defines n_intv
        inner = np.flatnonzero(touched)
        assert (np.diff(inner) > 1).sum() > 50                                 # untouched windows between touched ones
    got, want = check_index(ctx, recs, 1, "one reference")
    lin = got["linear"][3]
    assert len(lin) == 32768
    if not spanning:                                                           # a window no record touches carries the next touched one's offset
        gaps = np.flatnonzero(~touched[:-1])
        assert (lin[gaps] == lin[gaps + 1]).all() and lin[0] == lin[5] == len(HEAD) and lin[9000] == lin[32767] == want["runs"][2].max()


# ---- chunks at scale, from columns made here ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scale_case():
    """more than 1 024 blocks of the head scan (block_sums_scan_kernel folds two sums per lane) and several tiles of run keys.  The
    stream holds nothing but block_size words, of two sizes, so a chunk's end depends on its last record's own size."""
    rng = np.random.default_rng(4500)
    n, n_ref, n_tail = 1024 * 1024 + 1025, 3000, 5000
    ref = np.concatenate((np.sort(rng.integers(0, n_ref, n - n_tail)), np.full(n_tail, -1))).astype(np.int32)
    bins_of = rng.integers(0, 37449, (n_ref, 4))
    bin_ = np.where(ref >= 0, bins_of[np.maximum(ref, 0), rng.integers(0, 4, n)], 0).astype(np.int32)
    sizes = np.where(rng.integers(0, 2, n) == 1, 1000, 40).astype(np.int64)
    stream = HEAD + sizes.astype("<u4").tobytes()
    starts = len(HEAD) + 4 + 4 * np.arange(n, dtype=np.int64)
    want = bai.runs(ref, bin_, starts, sizes, n_ref)
    return dict(n_ref=n_ref, ref=ref, bin=bin_, stream=stream, starts=starts, sizes=sizes, want=want, n_runs=len(want[0]))


def test_chunks_at_scale(ctx, scale_case):
    c = scale_case
    w_ref, w_bin, w_beg, w_end = c["want"]
    assert (len(c["ref"]) + 1023) // 1024 == 1026 and c["n_runs"] > 2 * capi.SORT_TILE
    pair = w_ref.astype(np.int64) << 16 | w_bin
    again = np.flatnonzero(pair[1:] == pair[:-1])                           # one (ref, bin) as several runs: they must come out in file order
    assert len(again) > 1000 and (w_beg[again + 1] > w_beg[again]).all()
    assert w_ref[-1] == -1 and (w_ref == -1).sum() == 1 and set(np.unique(w_end - w_beg).tolist()) > {44, 1004}
    n_runs, *chunks = capi.bai_chunks(ctx, c["stream"], c["starts"], c["ref"], c["bin"], c["n_ref"])
    assert n_runs == c["n_runs"]
    check_chunks(chunks, c["want"], "scale")


@pytest.mark.parametrize("extra", [None, -1, 7], ids=["count_only", "cap_one_short", "cap_seven_more"])
def test_chunks_at_scale_with_a_cap(ctx, scale_case, extra):
    c = scale_case
    cap = 0 if extra is None else c["n_runs"] + extra
    n_runs, *chunks = capi.bai_chunks(ctx, c["stream"], c["starts"], c["ref"], c["bin"], c["n_ref"], cap=cap)
    assert n_runs == c["n_runs"] and all(len(a) == cap for a in chunks)
    if extra == -1:                                                         # too small: the count, and nothing written
        assert all(capi.untouched(a).all() for a in chunks)
    if extra == 7:
        check_chunks([a[:n_runs] for a in chunks], c["want"], "cap + 7")
        assert all(capi.untouched(a[n_runs:]).all() for a in chunks)


# ---- degenerate calls --------------------------------------------------------------------------------------------------------------------
def test_no_records(ctx):
    got, _ = check_index(ctx, [], 3, "no records")
    assert got["status"] == (0, -1, -1, 0) and all(len(a) == 0 for a in got["chunks"])
    n_intv, stat, lin_off, lin = got["linear"]
    assert n_intv.tolist() == [0, 0, 0] and stat[:2].tolist() == [[0, 0, 0], [0, 0, 0]] and lin_off.tolist() == [0, 0, 0, 0] and len(lin) == 0


def test_no_references(ctx):
    recs = [record(f"u{k}", 4, -1, -1, 0, "", l_seq=k % 5) for k in range(100)]
    got, want = check_index(ctx, recs, 0, "no references")
    assert got["status"] == (0, -1, -1, 100)
    assert [a.tolist() for a in got["chunks"]] == [[-1], [0], [len(HEAD)], [len(want["stream"])]]
    n_intv, stat, lin_off, lin = got["linear"]                              # (the wrapper found the guards of its empty arrays intact)
    assert len(n_intv) == 0 and stat.shape == (4, 0) and lin_off.tolist() == [0] and len(lin) == 0


def test_one_record(ctx):
    got, _ = check_index(ctx, [record("only", 16, 2, 40000, 60, "30M")], 5, "one record")
    assert got["linear"][0].tolist() == [0, 0, 3, 0, 0] and got["linear"][3].tolist() == [len(HEAD)] * 3
    check_index(ctx, [record("only", 4, -1, -1, 0, "", l_seq=3)], 5, "one unplaced record")


# ---- virtual offsets ---------------------------------------------------------------------------------------------------------------------
def member_table():
    """40 entries: two empty members in the middle, file offsets past 2^32 and up to 2^47"""
    rng = random.Random(4700)
    mu, mc = [1000], [0]
    for k in range(1, 40):
        mu.append(mu[-1] + (0 if k in (11, 26) else rng.randrange(1, 65281)))
        mc.append(mc[-1] + rng.randrange(28, 65536) if k < 8 else (1 << 32) - 25 + 10 * (k - 8) if k < 12 else mc[-1] + rng.randrange(1 << 30, 1 << 41))
    mc[-1] = 1 << 47
    assert all(a <= b for a, b in zip(mu, mu[1:])) and sum(a == b for a, b in zip(mu, mu[1:])) == 2 and all(a < b for a, b in zip(mc, mc[1:]))
    assert mc[10] < 1 << 32 <= mc[11] and max(b - a for a, b in zip(mu, mu[1:])) < 1 << 16
    return mu, mc


def test_virtual_offsets(ctx):
    mu, mc = member_table()
    rng = random.Random(4701)
    u = [v + d for v in mu for d in (-1, 0, 1)] + [mu[0] - 1, mu[-1] + 1, mu[-1], 0, -1, 1 << 40]
    u += [rng.randrange(mu[0], mu[-1] + 1) for _ in range(1000 - len(u))]
    rng.shuffle(u)
    want = bai.voffsets(u, mu, mc)
    by_u = dict(zip(u, want.tolist()))
    assert len(u) > 3 * 256 and by_u[mu[0] - 1] == by_u[mu[-1] + 1] == by_u[-1] == by_u[1 << 40] == bai.NONE
    assert by_u[mu[11]] == mc[11] << 16 and by_u[mu[26]] == mc[26] << 16 and by_u[mu[11] - 1] >> 16 == mc[9]    # of equal entries the LAST one
    assert by_u[mu[-1]] == 1 << 63 and by_u[mu[-1] - 1] == mc[-2] << 16 | (mu[-1] - 1 - mu[-2])
    same(capi.bgzf_voffsets(ctx, u, mu, mc), want, "voffsets")


def test_virtual_offsets_of_a_table_of_one_entry(ctx):
    u = [5000, 4999, 5001]
    want = bai.voffsets(u, [5000], [(1 << 33) + 7])
    assert want.tolist() == [((1 << 33) + 7) << 16, bai.NONE, bai.NONE]
    same(capi.bgzf_voffsets(ctx, u, [5000], [(1 << 33) + 7]), want, "one entry")
    assert len(capi.bgzf_voffsets(ctx, [], [5000], [7])) == 0
