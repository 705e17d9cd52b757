"""The arithmetic of the multi-GPU count-table exchange at the C ABI, against the exact numpy model of tests/eref_plane_cases.py:
palace_eref_table_merge_slices / _packed, _pack_low, palace_eref_plane_pack / _unpack, palace_eref_entry_hits_from_counts, and the two
hooks every other eref test leans on, palace_eref_table_lookup and _popcounts.  The planes are PLANTED -- written into the table's
device buffers and declared with palace_eref_table_invalidate -- not counted from reads, so every bit of every input is known; every
comparison is exact.  (The model itself is checked on a CPU: tests/test_host_eref_plane_model.py.)"""
import time

import numpy as np
import pytest

from oracle import binding as orc
from palace_amd import capi, multigpu, synth
from tests import eref_plane_cases as m

pytestmark = pytest.mark.gpu

PLANE = m.PLANE_BYTES
GUARD = 64                              # planted bytes on either side of a merged slice
GUARD_SLOTS = 1024                      # pre-filled entries behind the sparse form's counts / prefix arrays
FILL = 0xA5
KEY_FILL = 0xABCD
SHARES = {"b0": [0], "b127": [127], "r0of4": multigpu.key_buckets_of(0, 4), "r1of4": multigpu.key_buckets_of(1, 4),
          "r2of4": multigpu.key_buckets_of(2, 4), "r3of4": multigpu.key_buckets_of(3, 4), "all128": list(range(128))}


class World:
    """one context for the kernels under test, a second one for the receiving side of the sparse form, one small probe index"""

    def __init__(self):
        rng = synth.rng_for(4242)
        self.hdr = orc.header_from_picks(rng.integers(0, 6, size=32))
        self.ctx = capi.Ctx(0)
        self.ctx.eref_set_coder(self.hdr)
        self.other = capi.Ctx(0)
        self.other.eref_set_coder(self.hdr)
        refs = synth.reads_from_list([synth.random_dna(rng, n) for n in (3000, 700, 33, 1500)])
        self.rb, self.ro = self.ctx.upload(refs.bases), self.ctx.upload(refs.offsets)
        self.ix = self.ctx.eref_probe_index_build(self.rb, self.ro, refs.n, len(refs.bases))
        self.cb, self.hb = self.ctx.eref_entry_layout(self.ix)
        self.d_counts, self.d_hits = self.ctx.empty((self.cb,), np.uint8), self.ctx.empty((self.hb,), np.uint8)
        self.ctx.eref_entry_buffers_attach(self.ix, self.d_counts.ptr, self.d_hits.ptr)

    def close(self):
        self.ctx.eref_entry_buffers_attach(self.ix, None, None)
        self.ctx.eref_probe_index_free(self.ix)
        for b in (self.d_counts, self.d_hits, self.rb, self.ro):
            b.free()
        self.other.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


@pytest.fixture
def ctx(world):
    world.ctx.eref_table_reset()
    return world.ctx


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
        pytest.fail(f"{what}: {len(bad)} of {got.size} differ, first at {bad[:4].tolist()}: got {got.reshape(-1)[bad[:4]].tolist()}, "
                    f"want {want.reshape(-1)[bad[:4]].tolist()}")


def plant(ctx, off, planes):
    for p in range(3):
        ctx.eref_plane_write(p, off, planes[p])


def read3(ctx, off, n):
    return np.stack([ctx.eref_plane_read(p, off, n) for p in range(3)])


# ---- merges ---------------------------------------------------------------------------------------------------------------------
def merge_and_check(ctx, parts, slice_off, packed, seed, merged=None):
    """plant non-zero counts in the slice and GUARD bytes either side, merge `parts` (counts [n_parts][keys]) at slice_off, and compare:
    the slice is the fold of the parts ALONE, the guards are as planted, the popcounts say nothing else moved"""
    n_parts, slice_bytes = parts.shape[0], parts.shape[1] // 8
    lo, hi = max(0, slice_off - GUARD), min(PLANE, slice_off + slice_bytes + GUARD)
    before = m.nonzero_planes(np.random.default_rng(seed), hi - lo)
    plant(ctx, lo, before)
    d_parts = ctx.upload((m.packed_parts if packed else m.unary_parts)(parts))
    try:
        ctx.eref_table_merge_slices(d_parts.ptr, n_parts, slice_off, slice_bytes, packed=packed)
        got, pops = read3(ctx, lo, hi - lo), ctx.eref_table_popcounts()
    finally:
        d_parts.free()
    want = before.copy()
    want[:, slice_off - lo:slice_off - lo + slice_bytes] = m.planes_of_counts(m.merge_counts(parts)) if merged is None else merged
    for p in range(3):
        assert_same(got[p], want[p], f"plane {p} around the slice (byte 0 = plane offset {lo})")
    assert pops == [m.popcount(want[p]) for p in range(3)]


TRUTH_OFFS = (0, 16, 3 * m.TRUTH_PLANE_BYTES + 16, PLANE - m.TRUTH_PLANE_BYTES)


@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("slice_off", TRUTH_OFFS)
@pytest.mark.parametrize("n_parts", (1, 2, 3, 5, 8))
def test_merge_of_the_truth_table_slice(ctx, n_parts, slice_off, packed):
    """every combination of the parts' counts, 4^(8 - n_parts) times each, at the plane's start, off the 4 KiB grain, and at its end"""
    assert slice_off % 16 == 0 and slice_off + m.TRUTH_PLANE_BYTES <= PLANE
    merge_and_check(ctx, m.truth_parts(n_parts), slice_off, packed, seed=n_parts * 7 + int(packed))


@pytest.mark.parametrize("packed", (False, True))
@pytest.mark.parametrize("slice_bytes", (16, 16 * 257))
@pytest.mark.parametrize("slice_off_of", (lambda n: 0, lambda n: 16, lambda n: 3 * 8192 + 16, lambda n: PLANE - n), ids=("start", "off16", "off24592", "end"))
def test_merge_of_one_vector_and_of_a_block_and_a_vector(ctx, slice_off_of, slice_bytes, packed):
    for n_parts in (2, 3):
        ctx.eref_table_reset()
        parts = m.random_counts(np.random.default_rng(slice_bytes + n_parts), n_parts, slice_bytes * 8)
        merge_and_check(ctx, parts, slice_off_of(slice_bytes), packed, seed=slice_bytes + int(packed))


@pytest.mark.parametrize("packed", (False, True))
def test_merge_whose_second_grid_pass_is_short_and_not_block_aligned(ctx, packed):
    parts, merged = m.long_merge_case()
    slice_off = 5 * m.GRID_PASS_BYTES + 4096 + 48                    # no multiple of 4 KiB
    assert slice_off % 4096 and slice_off % 16 == 0
    merge_and_check(ctx, parts, slice_off, packed, seed=99, merged=merged)


@pytest.mark.parametrize("packed", (False, True))
def test_merge_of_nothing_and_refused_merges_change_nothing(ctx, packed):
    before = m.nonzero_planes(np.random.default_rng(3), 4096)
    plant(ctx, 0, before)
    plant(ctx, PLANE - 4096, before)
    pops = [2 * m.popcount(before[p]) for p in range(3)]
    d_parts = ctx.upload(np.zeros(3 * 3 * 32, np.uint8))
    try:
        ctx.eref_table_merge_slices(d_parts.ptr, 3, 16, 0, packed=packed)                  # an empty slice: OK, and nothing happens
        for n_parts, off, nbytes in ((3, 8, 16), (3, PLANE - 16, 32), (0, 16, 16), (3, 16, 24)):
            with pytest.raises(capi.PalaceError):
                ctx.eref_table_merge_slices(d_parts.ptr, n_parts, off, nbytes, packed=packed)
        assert_same(read3(ctx, 0, 4096), before, "the plane's start")
        assert_same(read3(ctx, PLANE - 4096, 4096), before, "the plane's end")
        assert ctx.eref_table_popcounts() == pops
    finally:
        d_parts.free()


# ---- pack_low -------------------------------------------------------------------------------------------------------------------
def test_pack_low_of_planted_counts_and_zero_everywhere_else(ctx):
    """truth-table and random counts at the plane's start, its end, and either side of the first grid pass's end (8 MiB); the whole
    low plane is read back and compared, byte by byte"""
    rng = np.random.default_rng(12)
    region = m.TRUTH_PLANE_BYTES + 4096
    want = np.zeros(PLANE, np.uint8)
    for i, off in enumerate((0, m.GRID_PASS_BYTES - region, m.GRID_PASS_BYTES, PLANE - region)):
        counts = np.concatenate([m.truth_parts(8)[2 * i + 1], rng.integers(0, 4, size=4096 * 8, dtype=np.uint8)])
        planes = m.planes_of_counts(counts)
        plant(ctx, off, planes)
        want[off:off + region] = m.low_plane(planes)
        assert_same(want[off:off + region], m.bits_to_bytes(counts & 1), "the model's two statements of the low bit")
    low = ctx.empty((PLANE + 16,), np.uint8)
    try:
        with pytest.raises(capi.PalaceError):
            ctx.eref_table_pack_low(low.ptr + 8)
        ctx.memset(low.ptr, FILL, PLANE + 16)
        t0 = time.perf_counter()
        ctx.eref_table_pack_low(low.ptr)
        got = low.to_host()
        print(f"pack_low + read-back of {PLANE >> 20} MiB: {time.perf_counter() - t0:.3f} s")
        t0 = time.perf_counter()
        assert (got[PLANE:] == FILL).all()
        assert_same(got[:PLANE], want, "low plane")
        print(f"comparison: {time.perf_counter() - t0:.3f} s")
    finally:
        low.free()


# ---- lookup and popcounts -------------------------------------------------------------------------------------------------------
EDGE_KEYS = (0, 31, 32, 63, 2**31 - 1, 2**31, 2**32 - 32, 2**32 - 1, 8 * m.GRID_PASS_BYTES - 1, 8 * m.GRID_PASS_BYTES)
EDGE_BASE = (1, 2, 3, 0, 3, 1, 2, 3, 2, 1)          # rotation r plants (base + r) % 4: over the four rotations every key holds every count


def plant_counts(ctx, counts_of: dict):
    """counts at single keys, written as whole 64-byte pieces of the three planes"""
    blocks = {}
    for k, c in counts_of.items():
        blocks.setdefault(k >> 9, np.zeros(512, np.uint8))[k & 511] = c
    for b, c in sorted(blocks.items()):
        plant(ctx, b * 64, m.planes_of_counts(c))


@pytest.mark.parametrize("n", (1, 255, 256, 257))
def test_lookup_and_popcounts_of_planted_keys(ctx, n):
    rng = np.random.default_rng(n)
    assert ctx.eref_table_popcounts() == [0, 0, 0]                  # the all-zero table
    assert not ctx.eref_table_lookup(np.array(EDGE_KEYS, np.uint32)).any()
    for rot in range(4):
        ctx.eref_table_reset()
        planted = {k: (c + rot) % 4 for k, c in zip(EDGE_KEYS, EDGE_BASE)}
        assert set(planted.values()) == {0, 1, 2, 3}
        plant_counts(ctx, planted)
        pool = sorted(set(k + d for k in EDGE_KEYS for d in (-1, 0, 1) if 0 <= k + d < 2**32))
        query = np.concatenate([rng.permutation(pool), rng.choice(pool, size=max(0, n - len(pool)))])[:n] if n > 1 else [EDGE_KEYS[7 - rot]]
        query = rng.permutation(np.asarray(query, dtype=np.uint64)).astype(np.uint32)
        assert len(query) == n and (n < len(pool) or set(query.tolist()) == set(pool))
        want = np.array([planted.get(int(k), 0) for k in query], np.uint8)
        assert_same(ctx.eref_table_lookup(query), want, f"lookup of {n} keys, rotation {rot}")
        assert ctx.eref_table_popcounts() == [sum(1 for c in planted.values() if c >= t) for t in (1, 2, 3)]


@pytest.mark.parametrize("plane", (0, 1, 2))
def test_popcounts_and_lookup_with_one_plane_alone_non_zero(ctx, plane):
    """not a unary table: the hooks only count bits"""
    data = np.random.default_rng(40 + plane).integers(0, 256, size=4096, dtype=np.uint8)
    off = m.GRID_PASS_BYTES - 2048                                   # across the end of the popcount grid's first pass
    ctx.eref_plane_write(plane, off, data)
    want = [0, 0, 0]
    want[plane] = m.popcount(data)
    assert ctx.eref_table_popcounts() == want
    keys = (8 * off + np.arange(8 * 4096, dtype=np.uint64)).astype(np.uint32)
    assert_same(ctx.eref_table_lookup(keys), m.bytes_to_bits(data), "lookup")


# ---- the sparse form of the ">= 3" plane ----------------------------------------------------------------------------------------
def plant_sparse(ctx, sparse):
    for f, keys in sparse.items():
        ctx.eref_plane_write(2, f * m.FINE_BYTES, m.fine_bytes(keys))


@pytest.mark.parametrize("share", SHARES.values(), ids=SHARES.keys())
def test_plane_pack_of_a_planted_plane(ctx, share):
    sparse = m.sparse_plane()
    plant_sparse(ctx, sparse)
    counts, first, keys = m.share_model(sparse, share)
    n, total = len(counts), len(keys)
    fine_of = m.share_fine_buckets(share)
    for cap in (total + 7, total, total - 1, 0):
        d_cnt = ctx.upload(np.full(n + GUARD_SLOTS, 0xA5A5A5A5, np.uint32))
        d_first = ctx.upload(np.full(n + 1 + GUARD_SLOTS, 0xA5A5A5A5A5A5A5A5, np.uint64))
        d_keys = ctx.upload(np.full(total + 16, KEY_FILL, np.uint16))
        try:
            ctx.eref_plane_pack(share, d_cnt.ptr, d_keys.ptr, cap, d_first.ptr)
            g_cnt, g_first, g_keys = d_cnt.to_host(), d_first.to_host(), d_keys.to_host()
        finally:
            for b in (d_cnt, d_first, d_keys):
                b.free()
        assert_same(g_cnt[:n], counts, f"counts (cap {cap})")
        assert (g_cnt[n:] == 0xA5A5A5A5).all(), "counts written behind the share's entries"
        assert_same(g_first[:n + 1], first, f"first (cap {cap})")
        assert int(g_first[n]) == total
        assert (g_first[n + 1:] == 0xA5A5A5A5A5A5A5A5).all(), "prefix entries written behind first[n]"
        room = min(cap, total)
        assert_same(g_keys[:room], keys[:room], f"keys (cap {cap})")
        assert (g_keys[room:] == KEY_FILL).all(), f"keys written at or beyond cap_keys = {cap}"
        full = (np.repeat(fine_of, g_cnt[:n]).astype(np.uint64)[:room] << np.uint64(16)) | g_keys[:room]
        assert (np.diff(full.astype(np.int64)) > 0).all()            # ascending inside and across buckets


def garbage_buckets(sparse, share):
    """fine buckets to fill with garbage before an unpack: inside the share (its first and last, ones with keys and ones without) and
    outside it (next to its level-1 buckets, and anywhere)"""
    fine_of = m.share_fine_buckets(share)
    with_keys = [int(f) for f in fine_of if int(f) in sparse]
    without = [int(f) for f in fine_of if int(f) not in sparse]
    inside = sorted(set([int(fine_of[0]), int(fine_of[-1])] + with_keys[:3] + with_keys[-2:] + without[:3] + without[-3:] + without[len(without) // 2:][:2]))
    outside = set()
    for b in share:
        outside |= {b * m.FINE_PER_L1 - 1, (b + 1) * m.FINE_PER_L1}
    outside |= {0, 1, m.N_FINE - 1, 40 * m.FINE_PER_L1 + 77}
    in_share = set(fine_of.tolist())
    return inside, sorted(f for f in outside if 0 <= f < m.N_FINE and f not in in_share)


@pytest.mark.parametrize("share", SHARES.values(), ids=SHARES.keys())
def test_plane_unpack_rewrites_its_share_and_nothing_else(world, share):
    other, sparse = world.other, m.sparse_plane()
    counts, first, keys = m.share_model(sparse, share)
    n, total = len(counts), len(keys)
    inside, outside = garbage_buckets(sparse, share)
    assert any(f in sparse for f in inside) and any(f not in sparse for f in inside) and (outside or len(share) == 128)
    rng = np.random.default_rng(len(share))
    garbage = {f: rng.integers(1, 256, size=m.FINE_BYTES, dtype=np.uint8) for f in inside + outside}
    outside_bits = sum(m.popcount(garbage[f]) for f in outside)
    d_cnt = other.upload(counts)
    d_first = other.upload(np.full(n + 1 + GUARD_SLOTS, 0xA5A5A5A5A5A5A5A5, np.uint64))
    try:
        for cap in (total, total // 2):
            other.eref_table_reset()
            for f, g in garbage.items():
                other.eref_plane_write(2, f * m.FINE_BYTES, g)
            d_keys = other.upload(np.concatenate([keys[:cap], np.full(1, KEY_FILL, np.uint16)]))
            try:
                other.eref_plane_unpack(share, d_cnt.ptr, d_keys.ptr, cap, d_first.ptr)
                want = m.share_cut(sparse, share, cap)                # fine bucket -> keys, for EVERY fine bucket of the share
                for f in sorted(set(inside) | set(f for f in want if len(want[f]) or f in sparse)):
                    assert_same(other.eref_plane_read(2, f * m.FINE_BYTES, m.FINE_BYTES), m.fine_bytes(want[f]), f"fine bucket {f} of the share (cap {cap})")
                for f in outside:
                    assert_same(other.eref_plane_read(2, f * m.FINE_BYTES, m.FINE_BYTES), garbage[f], f"fine bucket {f} outside the share (cap {cap})")
                # ... and no bit anywhere else: the totals leave room for none
                assert other.eref_table_popcounts() == [0, 0, min(cap, total) + outside_bits]
            finally:
                d_keys.free()
        with pytest.raises(capi.PalaceError):
            other.eref_plane_unpack([], d_cnt.ptr, d_cnt.ptr, 0, d_first.ptr)
        with pytest.raises(capi.PalaceError):
            other.eref_plane_pack([], d_cnt.ptr, d_cnt.ptr, 0, d_first.ptr)
    finally:
        d_cnt.free()
        d_first.free()
        other.eref_table_reset()


# ---- entry counts -> hit bits -----------------------------------------------------------------------------------------------------
def entry_parts(rng, n_parts, cb):
    """[n_parts][cb] bytes: random 2-bit counts everywhere, the truth-table block at the start and at the end of every part"""
    parts = rng.integers(0, 256, size=(n_parts, cb), dtype=np.uint8)
    truth = np.stack([m.entry_bytes(c) for c in m.truth_parts(n_parts)])
    parts[:, :m.TRUTH_ENTRY_BYTES] = truth
    parts[:, cb - m.TRUTH_ENTRY_BYTES:] = truth
    return parts


def hits_of(parts):
    return m.entry_hits(m.entries_of_bytes(parts))


@pytest.mark.parametrize("n_parts", (1, 3, 8))
def test_entry_hits_of_the_whole_block_and_rank_by_rank(world, n_parts):
    ctx, ix, cb, hb = world.ctx, world.ix, world.cb, world.hb
    assert cb == 2 * hb and cb % (16 * n_parts) == 0 and cb >= 2 * m.TRUTH_ENTRY_BYTES
    assert ctx.eref_entry_buffers(ix) == (world.d_counts.ptr, world.d_hits.ptr)
    parts = entry_parts(np.random.default_rng(n_parts), n_parts, cb)
    want = hits_of(parts)
    assert len(want) == hb
    d_parts = ctx.upload(parts)
    try:
        ctx.memset(world.d_hits.ptr, FILL, hb)
        ctx.eref_entry_hits_from_counts(ix, d_parts.ptr, n_parts, cb, 0, cb)
        assert_same(world.d_hits.to_host(), want, "hit bits of the whole block in one call")
    finally:
        d_parts.free()
    # rank by rank, as multigpu.merge_entry_counts passes it: the parts pointer is rank r's receive buffer [n_parts][S]
    S = cb // n_parts
    ctx.memset(world.d_hits.ptr, FILL, hb)
    for r in range(n_parts):
        d_recv = ctx.upload(np.ascontiguousarray(parts[:, r * S:(r + 1) * S]))
        try:
            ctx.eref_entry_hits_from_counts(ix, d_recv.ptr, n_parts, S, r * S, S)
            got = world.d_hits.to_host()
        finally:
            d_recv.free()
        assert_same(got[:(r + 1) * S // 2], want[:(r + 1) * S // 2], f"hit bits of the shares 0 .. {r}")
        assert (got[(r + 1) * S // 2:] == FILL).all(), f"rank {r} wrote behind its share"


@pytest.mark.parametrize("off,nbytes", ((16 * 3, 16), (16 * 5, 16 * 257), (16 * 1031, 16 * 257)))
def test_entry_hits_of_a_narrow_range_leave_the_rest_alone(world, off, nbytes):
    ctx, ix, cb, hb = world.ctx, world.ix, world.cb, world.hb
    parts = entry_parts(np.random.default_rng(off), 3, cb)
    want = np.full(hb, FILL, np.uint8)
    want[off // 2:(off + nbytes) // 2] = hits_of(parts[:, off:off + nbytes])
    d_parts = ctx.upload(parts)
    try:
        ctx.memset(world.d_hits.ptr, FILL, hb)
        ctx.eref_entry_hits_from_counts(ix, d_parts.ptr + off, 3, cb, off, nbytes)       # (part p's counts OF THE RANGE lie at ptr + p * stride)
        assert_same(world.d_hits.to_host(), want, "hit bits")
    finally:
        d_parts.free()


def test_entry_hits_refusals_write_nothing(world):
    ctx, ix, cb, hb = world.ctx, world.ix, world.cb, world.hb
    d_parts = ctx.upload(np.full((2, cb + 16), 0xFF, np.uint8))
    try:
        ctx.memset(world.d_hits.ptr, FILL, hb)
        for n_parts, stride, off, nbytes in ((2, cb, 8, 16), (2, cb, 16, 8), (2, cb + 8, 0, 16), (2, 16, 0, 32), (2, cb, cb - 16, 32), (0, cb, 0, 16)):
            with pytest.raises(capi.PalaceError):
                ctx.eref_entry_hits_from_counts(ix, d_parts.ptr, n_parts, stride, off, nbytes)
        ctx.eref_entry_hits_from_counts(ix, d_parts.ptr, 2, cb, 16, 0)                    # an empty range: OK, and nothing happens
        assert (world.d_hits.to_host() == FILL).all()
    finally:
        d_parts.free()


def test_entry_hits_of_a_count_block_longer_than_one_grid_pass(world):
    """a DB whose count block exceeds 8 MiB (2048 x 256 threads x 16 bytes): two parts of random counts over the whole block"""
    ctx = world.ctx
    rng = synth.rng_for(77)
    n_bases, ix = 9_600_000, None                                     # (grown until the block crosses: 19.5 units of 256 x 840 x 2 bytes make 8 MiB)
    bufs = []
    try:
        while True:
            t0 = time.perf_counter()
            refs = synth.reads_from_list([synth.random_dna(rng, n_bases)])
            rb, ro = ctx.upload(refs.bases), ctx.upload(refs.offsets)
            bufs += [rb, ro]
            ix = ctx.eref_probe_index_build(rb, ro, refs.n, len(refs.bases))
            cb, hb = ctx.eref_entry_layout(ix)
            print(f"DB of {n_bases} bases: count block of {cb} bytes, built in {time.perf_counter() - t0:.3f} s")
            if cb > m.GRID_PASS_BYTES:
                break
            ctx.eref_probe_index_free(ix)
            ix = None
            n_bases += 100_000
            assert n_bases < 12_000_000, "the layout arithmetic expects about 10 Mbases"
        d_counts, d_hits = ctx.empty((cb,), np.uint8), ctx.empty((hb,), np.uint8)
        bufs += [d_counts, d_hits]
        ctx.eref_entry_buffers_attach(ix, d_counts.ptr, d_hits.ptr)
        parts = entry_parts(np.random.default_rng(2), 2, cb)
        d_parts = ctx.upload(parts)
        bufs.append(d_parts)
        ctx.memset(d_hits.ptr, FILL, hb)
        ctx.eref_entry_hits_from_counts(ix, d_parts.ptr, 2, cb, 0, cb)
        assert_same(d_hits.to_host(), hits_of(parts), "hit bits")
    finally:
        if ix is not None:
            ctx.eref_entry_buffers_attach(ix, None, None)
            ctx.eref_probe_index_free(ix)
        for b in bufs:
            b.free()
