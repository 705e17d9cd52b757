"""palace_readqc_cycle_stats, palace_readqc_plan_ex and palace_readqc_insert_sizes (csrc/readqc.hip) through the C ABI against the numpy
restatement of tests/readqc_report_cases.py -- exactly, and never against the device's own output.  The sizes are the smallest at which
the kernels take another path: a wavefront's 64 cycles, the cycle tile, several tiles, more reads than workgroups."""
import numpy as np
import pytest

from palace_amd import capi, synth
from tests import readqc_cases as rc
from tests import readqc_report_cases as rr

pytestmark = pytest.mark.gpu

TILE = capi.READQC_CYCLE_TILE
BORDER_LENGTHS = (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1)


def random_reads(rng, lengths):
    """(name, seq, qual) per length: every base slot, QUAL bytes over the whole range with both borders of Q20 and Q30 frequent"""
    out = []
    for k, n in enumerate(lengths):
        seq = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=n, p=(0.28, 0.22, 0.22, 0.23, 0.05))]
        qual = rng.choice(np.array([33, 52, 53, 62, 63, 126] + list(range(34, 126)), np.uint8), size=n)
        out.append((b"r%d" % k, seq.tobytes(), qual.tobytes()))
    return out


def same(got, want, what):
    assert len(got) == len(want), what
    for s, (g, w) in enumerate(zip(got, want)):
        for k in ("cnt", "qsum"):
            bad = np.argwhere(g[k] != w[k])
            assert len(bad) == 0, (what, s, k, [(int(c), int(b), int(g[k][c, b]), int(w[k][c, b])) for c, b in bad[:6]])
        assert (g["q20"], g["q30"]) == (w["q20"], w["q30"]), (what, s)


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def test_cycle_stats_at_the_borders_of_a_wavefront_and_of_the_tile(ctx):
    rng = synth.rng_for(1)
    reads = random_reads(rng, BORDER_LENGTHS + BORDER_LENGTHS[::-1])
    text = rc.fastq(reads)
    lens = np.array([len(r[1]) for r in reads], np.int32)
    k = np.arange(len(reads))
    cut = np.where(k % 3 == 0, -1, np.where(k % 3 == 1, lens, np.maximum(lens - 1 - k, 0))).astype(np.int32)                  # dropped, whole and cut reads
    assert (cut == -1).sum() >= 5 and ((cut >= 0) & (cut < lens)).sum() >= 5 and (cut == lens).sum() >= 1
    qc = capi.Readqc(ctx, text, text)
    try:
        for max_cycles in (2 * TILE + 1, 2 * TILE, TILE + 1, TILE, TILE - 1, 65, 64, 1, 0):
            same(qc.cycle_stats(0, max_cycles, lens=cut), rr.cycle_stats(text, cut, max_cycles), ("after", max_cycles))
            same(qc.cycle_stats(1, max_cycles, after=False), rr.cycle_stats(text, None, max_cycles), ("d_len NULL", max_cycles))
        over = lens + 5                                                      # a kept length beyond the read counts the read, no more
        same(qc.cycle_stats(0, 2 * TILE + 1, lens=over), rr.cycle_stats(text, over, 2 * TILE + 1), "lengths beyond the reads")
    finally:
        qc.close()
    want = rr.cycle_stats(text, cut, 2 * TILE + 1)
    assert (want[0]["cnt"].sum(axis=0) > 0).all() and 0 < want[1]["q30"] < want[1]["q20"] < want[0]["q20"]


def test_cycle_stats_of_one_read_of_4096_bases(ctx):
    (read,) = random_reads(synth.rng_for(2), (rc.MAX_SEQ,))
    text = rc.fastq([read])
    qc = capi.Readqc(ctx, text, text)
    try:
        for lens in ([rc.MAX_SEQ], [rc.MAX_SEQ - 1], [-1]):
            same(qc.cycle_stats(0, rc.MAX_SEQ, lens=lens), rr.cycle_stats(text, lens, rc.MAX_SEQ), lens)
    finally:
        qc.close()


def test_cycle_stats_of_an_empty_text(ctx):
    qc = capi.Readqc(ctx, b"", b"")
    try:
        for max_cycles in (0, 1, TILE + 1):
            same(qc.cycle_stats(0, max_cycles, lens=[]), rr.cycle_stats(b"", [], max_cycles), max_cycles)
            same(qc.cycle_stats(0, max_cycles, after=False), rr.cycle_stats(b"", None, max_cycles), max_cycles)
    finally:
        qc.close()


def test_cycle_stats_of_more_reads_than_workgroups(ctx):
    """20 000 reads of up to 160 bases: the grid is at its cap, so every workgroup walks several steps of four reads"""
    rng = synth.rng_for(3)
    n = 20000
    lens = rng.integers(0, 161, size=n)
    lens[-3:] = (160, 0, 1)                                                  # the last step of the walk is not a full one for most workgroups
    reads = random_reads(rng, lens)
    text = rc.fastq(reads, last_lf=False)
    kept = np.where(rng.random(n) < 0.2, -1, np.where(rng.random(n) < 0.4, (lens * rng.random(n)).astype(np.int64), lens)).astype(np.int32)
    qc = capi.Readqc(ctx, text, text)
    try:
        same(qc.cycle_stats(0, 160, lens=kept), rr.cycle_stats(text, kept, 160), "20000 reads")
        same(qc.cycle_stats(1, 100, after=False), rr.cycle_stats(text, None, 100), "20000 reads, 100 cycles")
    finally:
        qc.close()


# ---- the candidates and the insert sizes ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded():
    """rc.random_pairs behind the hand-typed catalogue: texts, the restatement's plan, every pair's candidate and slot"""
    cat = rr.insert_catalogue()
    pairs = [(s1, bytes([70]) * len(s1), s2, bytes([70]) * len(s2)) for s1, s2, flags, _, _ in cat.values() if flags == "-"]
    by_hand = [(c, slot) for _, _, flags, c, slot in cat.values() if flags == "-"]
    rng = synth.rng_for(20261021)
    pairs += rc.random_pairs(rng, 3000)
    for _ in range(150):                                                     # fragments longer than a read: forward candidates at o >= 1
        s1, s2 = rc.pair_with_insert(rng, 150, 150, int(rng.integers(151, 270)))
        pairs.append((s1, bytes([70]) * 150, s2, bytes([70]) * 150))
    texts = rc.texts_of(pairs)
    facts = [rr.insert_size(p[0], p[2]) for p in pairs]
    assert facts[:len(by_hand)] == by_hand
    return texts, rc.readqc(*texts), np.array([f[0] for f in facts], np.int32), np.array([f[1] for f in facts]), len(by_hand)


def test_plan_ex_with_null_is_plan(ctx, seeded):
    texts, want, _, _, _ = seeded
    qc = capi.Readqc(ctx, *texts)
    try:
        for prm in (None, capi.ReadqcParams.default(no_trim=1)):
            old, new = qc.plan(prm), qc.plan_ex(prm, with_cand=False)
            assert set(old) == set(new)
            for k in old:
                assert np.array_equal(old[k], new[k]), k
        for k in ("len1", "len2", "off1", "off2"):                           # ... and what it was held to before
            assert np.array_equal(qc.plan_ex(with_cand=False)[k], want[k]), k
    finally:
        qc.close()


def test_plan_ex_candidates_and_insert_sizes(ctx, seeded):
    texts, want, cand, slots, n_hand = seeded
    hist = np.bincount(slots, minlength=rr.ISIZE_MAX + 1).astype(np.uint64)
    assert np.array_equal(hist, rr.insert_histogram(*texts))
    assert hist[rr.ISIZE_MAX] > 500 and hist[:150].sum() > 500 and hist[150:rr.ISIZE_MAX].sum() > 100 and hist[511] == 1 and (cand[want["len1"] < 0] >= 0).sum() > 50
    qc = capi.Readqc(ctx, *texts)
    try:
        got = qc.plan_ex()
        bad = np.nonzero(got["cand"] != cand)[0]
        assert len(bad) == 0, [(int(i), int(got["cand"][i]), int(cand[i])) for i in bad[:8]]
        for k in ("len1", "len2", "off1", "off2"):                           # the store changes nothing else
            assert np.array_equal(got[k], want[k]), k
        for k in rc.COUNTS:
            assert got[k] == want[k], k
        assert np.array_equal(qc.insert_sizes(), hist)
        assert np.array_equal(qc.insert_sizes(cand=cand), hist)              # ... and from the restatement's candidates
        off = capi.ReadqcParams.default(no_trim=1)
        assert np.all(qc.plan_ex(off)["cand"] == -1)                         # -A: no search, no candidate
        unknown = np.zeros(rr.ISIZE_MAX + 1, np.uint64)
        unknown[rr.ISIZE_MAX] = len(cand)
        assert np.array_equal(qc.insert_sizes(off), unknown)
    finally:
        qc.close()


def test_a_pair_that_is_not_staged_has_no_candidate(ctx):
    s1, s2 = rc.pair_with_insert(synth.rng_for(8), 100, 100, 80)
    good = (s1, b"I" * 100, s2, b"I" * 100)
    t1, t2 = rc.texts_of([good, good, good])
    t1 = t1.replace(b"I" * 100 + b"\n@p1", b"I" * 99 + b"\n@p1")            # pair 0: read 1's QUAL is one short (palace_fastq_records says so)
    qc = capi.Readqc(ctx, t1, t2)
    try:
        assert qc.records()[0][1:3] == (4, rc.EQLEN)
        got = qc.plan_ex()
        c = rr.insert_size(s1, s2)[0]
        assert c >= 0 and got["cand"].tolist() == [-1, c, c] and got["len1"].tolist() == [-1, 80, 80]
    finally:
        qc.close()


def test_no_pairs(ctx):
    qc = capi.Readqc(ctx, b"", b"")
    try:
        got = qc.plan_ex()
        assert len(got["cand"]) == 0 and got["reads_before"] == 0 and got["off1"].tolist() == [0]
        assert np.array_equal(qc.insert_sizes(), np.zeros(rr.ISIZE_MAX + 1, np.uint64))
    finally:
        qc.close()
