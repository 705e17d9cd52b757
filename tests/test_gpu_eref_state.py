"""What the count table accepts in each of its states, walked through the C ABI on a device: every call of tests/eref_state_cases.py
against every state, each on a freshly established state, compared with the one table of expectations (the state record itself on a
CPU: tests/test_host_eref_state.py).  And the merge after a partial count of no reads whose hit bits were declared whole: the indexed
scan must probe the merged planes for itself."""
import ctypes

import numpy as np
import pytest

from palace_amd import capi, synth
from tests import eref_state_cases as cases

pytestmark = pytest.mark.gpu

# what a refusal for the table's state says (anything else -- a bad argument, a HIP error -- is not a refusal but a broken test)
REFUSALS = ("the table holds only its \">= 3\" plane", "the table holds nothing", "one count call per reset",
            "is not attached to this context with option probe_all_sets 2", "no count call of this context has left its partial counts")
PLANE = 1 << 29


class World:
    """one context, one small sample, one DB with two builds of its probe index, and the buffers the calls work on"""

    def __init__(self):
        rng = synth.rng_for(1234)
        from oracle import binding as orc
        self.hdr = orc.header_from_picks(rng.integers(0, 6, size=32))
        refs = [synth.random_dna(rng, n) for n in (3000, 700, 33)]
        reads = [synth.mutate(rng, refs[0][s:s + 120], 0.005) for s in rng.integers(0, 3000 - 120, size=300)]
        rs, rr = synth.reads_from_list(reads), synth.reads_from_list(refs)
        self.n_reads, self.n_pos, self.n_refs, self.ref_bases = rs.n, len(rs.bases), rr.n, len(rr.bases)
        self.ctx = ctx = capi.Ctx(0)
        ctx.eref_set_coder(self.hdr)
        ctx.eref_set_count_mode(2, 0)                    # the binned kernels, although the input is tiny
        self.db, self.do = ctx.upload(rs.bases), ctx.upload(rs.offsets)
        self.rb, self.ro = ctx.upload(rr.bases), ctx.upload(rr.offsets)
        nb = int(capi.lib().palace_eref_packed_bytes(self.n_pos))
        self.streams = [ctx.upload(np.zeros(nb, np.uint8)) for _ in range(3)]
        ctx.eref_pack_reads(self.db, self.do, rs.n, None, self.n_pos, *self.streams)
        self.ix = ctx.eref_probe_index_build(self.rb, self.ro, self.n_refs, self.ref_bases)
        self.ix2 = ctx.eref_probe_index_build(self.rb, self.ro, self.n_refs, self.ref_bases)
        ctx.eref_entry_buffers_attach(self.ix, None, None)            # the index's own count block
        self.cb, _ = ctx.eref_entry_layout(self.ix)
        self.one_min, self.three_min = capi.window_minimums(0.9, 0.85)
        self.rows = ctx.empty((self.n_refs, 4), np.int32)
        self.zero_part = ctx.upload(np.zeros(48, np.uint8))           # [3][1][16] and [2][1][16]
        self.low = ctx.empty((PLANE,), np.uint8)
        self.keys10 = np.arange(10, dtype=np.uint32) * 0x01234567
        # a one-bucket sparse share (level-1 bucket 0: 512 fine buckets): what plane_pack fills, and the plain count's share for plane_unpack
        self.sp_out = [ctx.empty((512,), np.uint32), ctx.empty((1 << 16,), np.uint16), ctx.empty((513,), np.uint64)]
        self.sp_in = [ctx.empty((512,), np.uint32), ctx.empty((1 << 16,), np.uint16), ctx.empty((513,), np.uint64)]
        # the reference results, once: the plain count's rows, popcounts and sparse share
        self.establish("P")
        ctx.eref_plane_pack([0], self.sp_in[0].ptr, self.sp_in[1].ptr, 1 << 16, self.sp_in[2].ptr)
        self.pop = ctx.eref_table_popcounts()
        self.plain_rows = self.scan()
        assert self.pop[0] > self.pop[2] > 0 and self.plain_rows[0, 1] > 0 and not self.plain_rows[2, :2].any()      # keys reach 3; ref 0 is reported

    def close(self):
        ctx = self.ctx
        ctx.eref_attach_probe_index(None)
        ctx.eref_probe_index_free(self.ix)
        ctx.eref_probe_index_free(self.ix2)
        ctx.close()

    def count(self):
        self.ctx.eref_count_reads_packed(*self.streams, self.n_pos, self.n_reads)

    def establish(self, state):
        ctx = self.ctx
        ctx.eref_set_option("final_count", int(state not in "ZPU"))
        ctx.eref_set_option("probe_all_sets", 2 if state in cases.PARTIAL else 1 if state == "H" else 0)
        ctx.eref_attach_probe_index(self.ix if state in cases.ATTACHED else None)
        ctx.eref_table_reset()
        if state == "C0":
            capi._check(capi.lib().palace_eref_count_reads(ctx.h, None, None, 0, None, 0), "count of no reads")
        elif state != "Z":
            self.count()
        if state == "U":
            ctx.eref_table_invalidate()
        if state == "W":
            self.sum_own_counts()
            ctx.eref_entry_hits_complete(self.ix, 3 * self.n_pos)

    def sum_own_counts(self):
        """entry_hits_from_counts with one part, this context's own count block: the hit bits of what it counted alone"""
        counts, hits = ctypes.c_void_p(), ctypes.c_void_p()
        capi._check(capi.lib().palace_eref_entry_buffers(self.ix, ctypes.byref(counts), ctypes.byref(hits)), "palace_eref_entry_buffers")
        self.ctx.eref_entry_hits_from_counts(self.ix, counts.value, 1, self.cb, 0, self.cb)

    def scan(self, ix=None):
        ctx = self.ctx
        if ix is None:
            ctx.eref_scan_refs(self.rb, self.ro, self.n_refs, self.ref_bases, self.one_min, self.three_min, self.rows)
        else:
            ctx.eref_scan_refs_indexed(ix, self.rb, self.ro, self.n_refs, self.ref_bases, self.one_min, self.three_min, self.rows)
        return self.rows.to_host().copy()

    def call(self, name):
        ctx = self.ctx
        if name == "count_reads":
            ctx.eref_count_reads(self.db, self.do, self.n_reads, None, self.n_pos)
        elif name == "count_reads_packed":
            self.count()
        elif name in ("merge_slices", "merge_slices_packed"):
            ctx.eref_table_merge_slices(self.zero_part.ptr, 1, 0, 16, packed=name.endswith("packed"))
        elif name == "pack_low":
            ctx.eref_table_pack_low(self.low.ptr)
        elif name == "lookup":
            return ctx.eref_table_lookup(self.keys10)
        elif name == "table_planes":
            return ctx.eref_table_planes()
        elif name == "plane_pack":
            ctx.eref_plane_pack([0], self.sp_out[0].ptr, self.sp_out[1].ptr, 1 << 16, self.sp_out[2].ptr)
        elif name == "plane_unpack":
            ctx.eref_plane_unpack([0], self.sp_in[0].ptr, self.sp_in[1].ptr, 1 << 16, self.sp_out[2].ptr)
        elif name == "popcounts":
            return ctx.eref_table_popcounts()
        elif name == "scan_refs":
            return self.scan()
        elif name == "scan_refs_indexed":
            return self.scan(self.ix)
        elif name == "scan_refs_indexed_other":
            return self.scan(self.ix2)
        elif name == "entry_hits_complete":
            ctx.eref_entry_hits_complete(self.ix, 3 * self.n_pos)
        elif name == "reset":
            ctx.eref_table_reset()
        elif name == "invalidate":
            ctx.eref_table_invalidate()
        else:
            assert name == "attach_probe_index_null", name
            ctx.eref_attach_probe_index(None)
        ctx.sync()
        return None


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.mark.parametrize("state", cases.STATES)
def test_every_call_is_accepted_or_refused_as_the_table_says(world, state):
    observed = {}
    for name, accepting in cases.ACCEPTED.items():
        world.establish(state)
        before = world.scan(world.ix) if state in cases.ROWS_SURVIVE_REFUSALS else None
        try:
            result = world.call(name)
            observed[name] = True
        except capi.PalaceError as e:
            assert any(text in str(e) for text in REFUSALS), (state, name, str(e))
            observed[name] = False
            if before is not None:                       # the refused call changed nothing: the same rows, and they are the plain count's
                assert np.array_equal(world.scan(world.ix), before), (state, name)
        print(f"state {state:2s} {name:24s} {'accepted' if observed[name] else 'refused'}")
        if before is not None:
            assert np.array_equal(before, world.plain_rows), state
        if observed[name] and name == "popcounts":
            assert result == ([0, 0, world.pop[2]] if state in cases.TOP_ONLY else [0, 0, 0] if state in ("Z", "C0") else world.pop), (state, result)
        if observed[name] and name.startswith("scan_refs") and state in ("P", "U", "T", "T0", "H", "W"):
            assert np.array_equal(result, world.plain_rows), (state, name)
    assert observed == {name: state in accepting for name, accepting in cases.ACCEPTED.items()}, state


def test_a_merge_after_hit_bits_declared_whole_makes_the_scan_probe_for_itself(world):
    """A rank without reads (partial count of no reads, its zero counts summed into the hit bits), the hit bits declared whole, then a
    merge of whole planes: the merge writes the planes, so the record of the hit bits is dropped and the indexed scan probes the merged
    planes -- the rows of the plain count.  (Without the sum the hit-bit block would hold what the walk of the matrix left there, the
    right hits of this very sample, and a scan that wrongly started from them would pass.)"""
    ctx = world.ctx
    world.establish("P")
    planes, nbytes = ctx.eref_table_planes()
    assert nbytes == PLANE
    part = ctx.empty((3 * PLANE,), np.uint8)                           # [3][1][plane]
    try:
        for p in range(3):
            ctx.d2d(part.ptr + p * PLANE, planes[p], PLANE)
        world.establish("C0")
        world.sum_own_counts()                                         # (all zero: the hit bits of a sample without reads, whatever the block held)
        ctx.eref_entry_hits_complete(world.ix, -1)
        assert not world.scan(world.ix)[:, :2].any()                   # the scan starts from them: nothing is reported
        ctx.eref_table_merge_slices(part.ptr, 1, 0, PLANE)
        assert np.array_equal(world.scan(world.ix), world.plain_rows)
        assert ctx.eref_table_popcounts() == world.pop
    finally:
        ctx.sync()
        part.free()
