"""The count partition of eref (eref_bin1_sort_kernel -> eref_bin2_kernel -> eref_lds_count_kernel) on the planted read sets of
tests/eref_key_cases.py: every case sits on one capacity edge (a claim the host test asserts) and goes through the direct and
the binned kernels, the ASCII and the packed entry, its P = 8 and its P = 6 form, the whole key space, the share of the planted
buckets and its complement, a plain count, a second count on the table the first left, and a final count
(which with several slabs is a plain count).  Bit-exact against the
oracle's counts: a look-up of every key and its neighbours, and the three plane totals (a stray bit anywhere fails).

Which instantiation runs where (kernel<template arguments>):
  eref_bin1_sort_kernel<8, 512, false> / <6, 512, false>   every case, P = 8 / P = 6 form, whole key space
  eref_bin1_sort_kernel<8, 512, true>  / <6, 512, true>    every case, P = 8 / P = 6 form, the share and its complement
  eref_lds_count_kernel<true>          first count call of a binned run
  eref_lds_count_kernel<false>         second count call of a binned run; the second slab of the `slab` cases
  eref_lds_count_kernel<true, true>    the final count of a binned run (its n8 == 0 branch: every bucket of the cases with cap 1)
"""
import numpy as np
import pytest

from palace_amd import capi
from tests import eref_key_cases as kc

pytestmark = pytest.mark.gpu

CAT = kc.catalogue()
SLICE_BYTES = (1 << kc.FINE_SHIFT) // 8                     # a fine bucket's part of one plane


@pytest.fixture(scope="module")
def ctx():
    c = capi.Ctx(0)
    c.eref_set_coder(CAT.header)
    yield c
    c.close()


def _neighbours(u):
    u = u.astype(np.uint32)
    return np.unique(np.concatenate([u, u + np.uint32(1), u - np.uint32(1), u ^ np.uint32(1 << 16), u ^ np.uint32(1 << 25)]))


def _want(probes, u, n):
    """the oracle's count of every probe: n where the probe is a key, 0 elsewhere"""
    out = np.zeros(len(probes), np.uint8)
    if len(u):
        at = np.minimum(np.searchsorted(u, probes), len(u) - 1)
        hit = u[at] == probes
        out[hit] = n[at[hit]]
    return out


def _assert_table(ctx, probes, u, n, where):
    got = ctx.eref_table_lookup(probes)
    want = _want(probes, u, n)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (where, len(bad), [(hex(int(probes[i])), int(got[i]), int(want[i])) for i in bad[:8]])
    assert ctx.eref_table_popcounts() == [int((n >= 1).sum()), int((n >= 2).sum()), int((n >= 3).sum())], where


def _assert_final(ctx, u, n, where):
    """after a final count: the two lower planes all zero (touched buckets included), plane 3 exactly the keys counted three times
    (the total is right and every expected bit is set: the same set)"""
    top = u[n >= 3]
    assert ctx.eref_table_popcounts() == [0, 0, len(top)], where
    for fb in np.unique(top >> kc.FINE_SHIFT).tolist():
        words = ctx.eref_plane_read(2, fb * SLICE_BYTES, SLICE_BYTES).view(np.uint32)
        k = top[top >> kc.FINE_SHIFT == fb] & np.uint32(0xffff)
        assert np.all((words[k >> 5] >> (k & 31)) & 1), (where, fb)


def _run_form(ctx, case, P):
    f = CAT.form(case.name, P)
    case.claim(f)                                                                  # the input sits on the edge it is named after
    rs = f.rs
    n_pos = len(rs.bases)
    db, do = ctx.upload(rs.bases), ctx.upload(rs.offsets)
    ds = [ctx.upload(np.zeros(int(capi.lib().palace_eref_packed_bytes(n_pos)), np.uint8)) for _ in range(3)]
    ctx.eref_pack_reads(db, do, rs.n, None, n_pos, ds[0], ds[1], ds[2])
    ctx.sync()
    probes = _neighbours(f.expected()[0])
    own = sorted(case.buckets)
    shares = (("whole", None), ("share", own), ("complement", [b for b in range(kc.L1_BUCKETS) if b not in own]))

    def count(entry):
        if entry == "ascii":
            ctx.eref_count_reads(db, do, rs.n)
        else:
            ctx.eref_count_reads_packed(ds[0], ds[1], ds[2], n_pos, rs.n)         # (the hint: the same P as the ASCII entry picks)

    try:
        for mode in (1, 2):                                                        # the direct kernels / the partition kernels
            ctx.eref_set_count_mode(mode, case.cap if mode == 2 else 0)
            ctx.eref_set_option("slab_bases", case.slab if mode == 2 else 0)
            for tag, share in shares:
                ctx.eref_set_key_buckets(share)
                for entry in ("ascii", "packed"):
                    where = (case.name, P, mode, tag, entry)
                    ctx.eref_table_reset()
                    count(entry)
                    _assert_table(ctx, probes, *f.expected(share), where + ("clean",))
                    count(entry)                                                   # the table the first call left: not clean
                    _assert_table(ctx, probes, *f.expected(share, times=2), where + ("second call",))
                    if mode == 2:
                        try:
                            ctx.eref_set_option("final_count", 1)
                            ctx.eref_table_reset()
                            count(entry)
                            if f.n_slabs == 1:
                                _assert_final(ctx, *f.expected(share), where + ("final",))
                            else:                                                  # (the option applies to counts of one slab: include/palace_hip.h)
                                _assert_table(ctx, probes, *f.expected(share), where + ("final, several slabs: a plain count",))
                        finally:
                            ctx.eref_set_option("final_count", 0)
                            ctx.eref_table_reset()
    finally:
        ctx.eref_set_key_buckets(None)
        ctx.eref_set_option("final_count", 0)
        ctx.eref_set_option("slab_bases", 0)
        ctx.eref_set_count_mode(0, 0)
        ctx.eref_table_reset()
        for b in [db, do] + ds:
            b.free()
        if case.big:
            CAT.drop(case.name)


@pytest.mark.parametrize("P", kc.FORMS)
@pytest.mark.parametrize("name", [c.name for c in CAT.cases])
def test_planted_case_equals_the_oracle_through_every_path(ctx, name, P):
    _run_form(ctx, CAT.by_name[name], P)
