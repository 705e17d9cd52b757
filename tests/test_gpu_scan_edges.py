"""Phase B of eref (palace_eref_scan_refs, palace_eref_scan_refs_indexed) on planted per-channel hit patterns that sit on the
edges of its pruning rules -- sentinel pruning, cheap exclusion, chunk need, two-stage pruning, the edge list and its serial walk,
the multi-sweep prefix -- through every device path, bit for bit against tests/scan_cases.rows_model over the oracle's bits.
The catalogue and what each case claims are in tests/scan_cases.py; tests/test_host_scan_cases.py pins the model to the oracle."""
from types import SimpleNamespace

import numpy as np
import pytest

from palace_amd import capi, synth
from tests import scan_cases as sc

pytestmark = pytest.mark.gpu

FORMS = ["catalogue", "reversed", "single_sentinel", "single_many_edges", "single_long"]


@pytest.fixture(scope="module")
def dev():
    cat = sc.catalogue()
    ctx = capi.Ctx(0)
    ctx.eref_set_coder(cat.header)
    rr = cat.reads_thrice()                                    # a hit needs count 3; one count call takes them all (the fused paths)
    d = SimpleNamespace(cat=cat, ctx=ctx, rb=ctx.upload(rr.bases), ro=ctx.upload(rr.offsets), n_reads=rr.n, dbs={})
    for form, order in cat.db_forms().items():
        rs = synth.reads_from_list([cat.refs[g] for g in order])
        d.dbs[form] = SimpleNamespace(form=form, order=order, bases=ctx.upload(rs.bases), offsets=ctx.upload(rs.offsets), n=rs.n,
                                      total=len(rs.bases), rows=ctx.empty((rs.n, 4), np.int32), ix=None,
                                      lens=np.array([len(cat.refs[g]) for g in order], dtype=np.int32))
    try:
        yield d
    finally:
        for db in d.dbs.values():
            if db.ix is not None:
                ctx.eref_probe_index_free(db.ix)
            for b in (db.bases, db.offsets, db.rows):
                b.free()
        d.rb.free(); d.ro.free()
        ctx.close()


def index_of(dev, db):
    if db.ix is None:
        db.ix = dev.ctx.eref_probe_index_build(db.bases, db.offsets, db.n, db.total)
    return db.ix


def count_plain(dev):
    dev.ctx.eref_set_count_mode(0, 0)
    dev.ctx.eref_table_reset()
    dev.ctx.eref_count_reads(dev.rb, dev.ro, dev.n_reads)


def check_rows(dev, db, T1, T3, path, lo=0, hi=None):
    """the rows the last scan left against the model: (n_intervals, el) for the refs [lo, hi) of the DB, zero outside; len; 0.
    -> the refs that differ, as text"""
    got = db.rows.to_host()
    hi = db.n if hi is None else hi
    want = np.zeros((db.n, 2), dtype=np.int32)
    for k in range(lo, hi):
        want[k] = dev.cat.rows(db.order[k], T1, T3)[:2]
    assert np.array_equal(got[:, 2], db.lens) and not got[:, 3].any(), (path, db.form, T1, T3)
    return [f"{dev.cat.case_of[db.order[k]].name} under {(T1, T3)}: got {got[k, :2].tolist()}, want {want[k].tolist()}"
            for k in np.flatnonzero((got[:, :2] != want).any(axis=1))]


def scan_all_pairs(dev, db, path, indexed, lo=0, hi=None):
    """every threshold pair of the catalogue through one path; every ref of the DB must equal the model under every pair"""
    ctx = dev.ctx
    bad = []
    for T1, T3 in dev.cat.pairs:
        if indexed:
            ctx.eref_scan_refs_indexed(index_of(dev, db), db.bases, db.offsets, db.n, db.total, T1, T3, db.rows)
        else:
            ctx.eref_scan_refs(db.bases, db.offsets, db.n, db.total, T1, T3, db.rows)
        bad += check_rows(dev, db, T1, T3, path, lo, hi)
    assert not bad, (path, db.form, (lo, hi), f"{len(bad)} (ref, pair) rows differ", bad[:12])


@pytest.mark.parametrize("form", FORMS)
def test_plain(dev, form):
    """eref_count_reads, then eref_scan_refs: channel 0 recomputed from the bases, pruned with the exact three_min"""
    count_plain(dev)
    scan_all_pairs(dev, dev.dbs[form], "plain", indexed=False)


@pytest.mark.parametrize("form", FORMS)
def test_indexed(dev, form):
    """the same table, the indexed scan probing for itself; the table is sparse: sentinel pruning alone"""
    count_plain(dev)
    scan_all_pairs(dev, dev.dbs[form], "indexed", indexed=True)


@pytest.mark.parametrize("form", FORMS)
def test_indexed_dense(dev, form):
    """... after eref_table_invalidate: sentinel pruning, then channel 0 pruned with the exact three_min, then channels 1 and 2"""
    count_plain(dev)
    try:
        dev.ctx.eref_table_invalidate()
        scan_all_pairs(dev, dev.dbs[form], "indexed_dense", indexed=True)
    finally:
        dev.ctx.eref_table_reset()


def fused(dev, db, cap, all_sets, path):
    ctx = dev.ctx
    try:
        ctx.eref_set_count_mode(2, cap)
        ctx.eref_attach_probe_index(index_of(dev, db))
        ctx.eref_set_option("final_count", 1)
        ctx.eref_set_option("probe_all_sets", 1 if all_sets else 0)
        ctx.eref_table_reset()
        ctx.eref_count_reads(dev.rb, dev.ro, dev.n_reads)
        scan_all_pairs(dev, db, path, indexed=True)
    finally:
        ctx.eref_attach_probe_index(None)
        ctx.eref_set_option("final_count", 0)
        ctx.eref_set_option("probe_all_sets", 0)
        ctx.eref_set_count_mode(0, 0)
        ctx.eref_table_reset()


@pytest.mark.parametrize("cap", [0, 64])
@pytest.mark.parametrize("form", FORMS)
def test_fused_c0(dev, form, cap):
    """the binned count with the index attached as the final count: channel 0's hit bits come from the count launch"""
    fused(dev, dev.dbs[form], cap, False, f"fused_c0/{cap}")


@pytest.mark.parametrize("cap", [0, 64])
@pytest.mark.parametrize("form", FORMS)
def test_fused_all(dev, form, cap):
    """... plane-less: all four entry sets come from the count launch, the sentinels already in position order"""
    fused(dev, dev.dbs[form], cap, True, f"fused_all/{cap}")


def range_cuts(dev, db):
    """[lo, hi) in DB order: between families, inside families, up to the end, nothing"""
    if db.n == 1:
        return [(0, 1), (1, 1)]
    cat = dev.cat
    pos = {g: k for k, g in enumerate(db.order)}
    first = {}
    for c in cat.cases:
        first.setdefault(c.family, c.first)
    named = [(first["exact"], first["far_chunk"]), (cat.index_of("sentinel/T400_a642_short"), cat.index_of("long/131073")),
             (cat.index_of("many_edges/1024"), cat.index_of("degenerate_db/copies") + 1)]
    cuts = [tuple(sorted((pos[a], pos[b]))) for a, b in named]
    return cuts + [(cuts[0][0], db.n), (0, cuts[1][1]), (5, 5)]


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("form", FORMS)
def test_range(dev, form, dense):
    """options scan_ref_lo / scan_ref_hi: the rows of the refs inside equal the model, those outside are zero"""
    ctx, db = dev.ctx, dev.dbs[form]
    count_plain(dev)
    try:
        if dense:
            ctx.eref_table_invalidate()
        for lo, hi in range_cuts(dev, db):
            ctx.eref_set_option("scan_ref_lo", lo)
            assert hi > 0                                                   # (0 would mean "up to the end")
            ctx.eref_set_option("scan_ref_hi", hi)
            scan_all_pairs(dev, db, "range", indexed=True, lo=lo, hi=hi)
    finally:
        ctx.eref_set_option("scan_ref_lo", 0)
        ctx.eref_set_option("scan_ref_hi", 0)
        ctx.eref_table_reset()
