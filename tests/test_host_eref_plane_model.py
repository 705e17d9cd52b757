"""The numpy model of the count-table exchange (tests/eref_plane_cases.py) must not rest on itself: it equals a second statement written
from the wording of include/palace_hip.h, its truth-table slice holds every combination of the parts' counts the stated number of
times, the planted sparse plane holds every edge the device tests name, and the packed form satisfies its identities.  No GPU."""
import numpy as np
import pytest

from palace_amd import multigpu
from tests import eref_plane_cases as m

GPU_N_PARTS = (1, 2, 3, 5, 8)           # what tests/test_gpu_eref_exchange_math.py merges on the truth-table slice
GPU_ENTRY_PARTS = (1, 3, 8)             # ... and sums as entry counts


def fold_pairwise(parts):
    """the header's wording: the saturating add (a + b >= t for t = 1, 2, 3) on integer counts, folded over the parts pairwise"""
    acc = np.zeros(parts.shape[1], dtype=np.int64)
    for b in parts:
        s = acc + b.astype(np.int64)
        acc = (s >= 1).astype(np.int64) + (s >= 2) + (s >= 3)            # the clamp: a count is the number of thresholds it reaches
    return acc.astype(np.uint8)


@pytest.mark.parametrize("n_parts", (1, 2, 3, 4, 5, 8))
def test_truth_table_slice_holds_every_combination_equally_often(n_parts):
    parts = m.truth_parts(n_parts)
    assert parts.shape == (n_parts, m.TRUTH_KEYS) and parts.max() == 3
    hist = m.combination_histogram(parts)
    assert len(hist) == 4 ** n_parts and (hist == 4 ** (8 - n_parts)).all()


def test_truth_table_outcomes_with_eight_parts():
    merged = m.merge_counts(m.truth_parts(8))
    assert np.bincount(merged, minlength=4).tolist() == [1, 8, 36, 65491]


def test_the_device_tests_use_covered_part_counts():
    assert set(GPU_N_PARTS) | set(GPU_ENTRY_PARTS) <= {1, 2, 3, 4, 5, 8}


@pytest.mark.parametrize("n_parts", sorted(set(GPU_N_PARTS) | set(GPU_ENTRY_PARTS)))
def test_merge_equals_the_pairwise_fold_of_the_header(n_parts):
    rng = np.random.default_rng(n_parts)
    for parts in (m.truth_parts(n_parts), m.random_counts(rng, n_parts, 16 * 257 * 8)):
        want = fold_pairwise(parts)
        assert np.array_equal(m.merge_counts(parts), want)
        # ... and through the bytes the kernels take, both forms: decode every part, fold, compare the planes
        un = m.unary_parts(parts)
        assert un.shape == (3, n_parts, parts.shape[1] // 8)
        decoded = np.stack([m.counts_of_planes(un[:, p]) for p in range(n_parts)])
        assert np.array_equal(decoded, parts)
        pk = m.packed_parts(parts)
        assert pk.shape == (2, n_parts, parts.shape[1] // 8)
        decoded = np.stack([m.bytes_to_bits(pk[0, p]) + 2 * m.bytes_to_bits(pk[1, p]) for p in range(n_parts)])
        assert np.array_equal(decoded, parts)
        assert np.array_equal(m.planes_of_counts(want), np.stack([m.bits_to_bytes(want >= t) for t in (1, 2, 3)]))


def test_bit_layout_is_little_endian_words():
    c = np.zeros(64, np.uint8)
    c[[0, 31, 32, 63]] = (1, 2, 3, 1)
    planes = m.planes_of_counts(c)
    words = planes.view("<u4")
    assert words[0].tolist() == [(1 << 0) | (1 << 31), (1 << 0) | (1 << 31)]
    assert words[1].tolist() == [1 << 31, 1 << 0]
    assert words[2].tolist() == [0, 1 << 0]
    assert np.array_equal(m.counts_of_planes(planes), c)


@pytest.mark.parametrize("n_parts", GPU_N_PARTS)
def test_packed_identities(n_parts):
    rng = np.random.default_rng(100 + n_parts)
    for parts in (m.truth_parts(n_parts), m.random_counts(rng, n_parts, 4096)):
        un, pk = m.unary_parts(parts), m.packed_parts(parts)
        p1, p2, p3 = un
        low, high = pk
        assert np.array_equal(low | high, p1) and np.array_equal(low & high, p3) and np.array_equal(high, p2)
        assert np.array_equal(low, p1 ^ p2 ^ p3)
        for p in range(n_parts):
            assert np.array_equal(m.low_plane(un[:, p]), low[p])


def test_nonzero_planes_are_unary_and_nowhere_zero():
    planes = m.nonzero_planes(np.random.default_rng(5), 4096)
    assert (planes[0] == 0xFF).all() and ((planes[1] & ~planes[0]) == 0).all() and ((planes[2] & ~planes[1]) == 0).all()
    assert sorted(np.unique(m.counts_of_planes(planes)).tolist()) == [1, 2, 3]


@pytest.mark.parametrize("n_parts", GPU_ENTRY_PARTS)
def test_entry_hits_equal_a_walk_over_the_two_bit_fields(n_parts):
    rng = np.random.default_rng(200 + n_parts)
    for parts in (m.truth_parts(n_parts), m.random_counts(rng, n_parts, 16 * 257 * 4)):
        blocks = np.stack([m.entry_bytes(c) for c in parts])
        assert blocks.shape == (n_parts, parts.shape[1] // 4)
        assert np.array_equal(m.entries_of_bytes(blocks), parts)
        # second statement: u16 by u16 as the header words it -- eight entries per 16 bits, hit bit e of byte j for entry 8 j + e
        u16 = blocks.view("<u2").astype(np.int64)
        want = np.zeros(u16.shape[1], dtype=np.uint8)
        for e in range(8):
            total = sum((u16[p] >> (2 * e)) & 3 for p in range(n_parts))
            want |= ((total >= 3).astype(np.uint8) << e).astype(np.uint8)
        assert np.array_equal(m.entry_hits(parts), want)
    # the truth-table block: every combination of the parts' counts is there, and the outcome is the merge's top plane
    parts = m.truth_parts(n_parts)
    assert (m.combination_histogram(parts) == 4 ** (8 - n_parts)).all()
    assert np.array_equal(m.entry_hits(parts), m.planes_of_counts(m.merge_counts(parts))[2])


def test_long_merge_case_crosses_one_grid_pass_by_a_block_and_a_vector():
    parts, merged = m.long_merge_case()
    nbytes = merged.shape[1]
    assert nbytes == 8 * 1024 * 1024 + 16 * 257 and parts.shape == (2, nbytes * 8)
    assert (m.combination_histogram(parts[:, :1 << 16]) > 0).all()
    head = slice(0, 4096 * 8)
    assert np.array_equal(m.planes_of_counts(fold_pairwise(parts[:, head])), merged[:, :4096])
    tail = slice((nbytes - 4096) * 8, nbytes * 8)
    assert np.array_equal(m.planes_of_counts(fold_pairwise(parts[:, tail])), merged[:, -4096:])


def test_sparse_plane_holds_every_edge_the_device_tests_name():
    sp = m.sparse_plane()
    full = [f for f, k in sp.items() if len(k) == m.FINE_KEYS]
    assert full and all(np.array_equal(sp[f], np.arange(m.FINE_KEYS)) and sp[f][-1] == 0xFFFF for f in full)
    assert any(sp[f].tolist() == [0] for f in sp) and any(sp[f].tolist() == [0xFFFF] for f in sp)
    assert any(sp[f].tolist() == [255, 256, 16383, 16384] for f in sp)
    assert sum(1 for k in sp.values() if 1 < len(k) < m.FINE_KEYS and len(k) != 4) >= 200            # "a few hundred random ones"
    assert 0 in sp and m.N_FINE - 1 in sp
    edges = [f for f in sp if f % m.FINE_PER_L1 == m.FINE_PER_L1 - 1 and f + 1 in sp]
    assert edges, "the last fine bucket of a level-1 bucket together with the first of the next"
    # ... once with the two level-1 buckets in different shares of four ranks
    owner = {b: r for r in range(4) for b in multigpu.key_buckets_of(r, 4)}
    assert any(owner[f // m.FINE_PER_L1] != owner[(f + 1) // m.FINE_PER_L1] for f in edges)
    for keys in sp.values():
        assert keys.dtype == np.uint16 and (np.diff(keys.astype(np.int64)) > 0).all()
    # every share the device tests use has keys, and fine buckets without any
    for share in [[0], [127]] + [multigpu.key_buckets_of(r, 4) for r in range(4)] + [list(range(128))]:
        counts, first, keys = m.share_model(sp, share)
        assert len(counts) == 512 * len(share) and len(first) == len(counts) + 1 and int(first[-1]) == len(keys) == int(counts.sum()) > 1
        assert (counts == 0).any() and first[0] == 0
    counts, first, keys = m.share_model(sp, range(128))
    assert len(keys) == sum(len(k) for k in sp.values())


def test_share_model_equals_a_walk_over_the_plane_bytes():
    """second statement of the sparse form: set the bits in the bytes of a level-1 bucket, then read counts and keys off the bytes"""
    sp = m.sparse_plane()
    for b in (0, 127):
        plane = np.zeros(m.FINE_PER_L1 * m.FINE_BYTES, np.uint8)
        for f, keys in sp.items():
            if f // m.FINE_PER_L1 == b:
                at = (f % m.FINE_PER_L1) * m.FINE_BYTES
                plane[at:at + m.FINE_BYTES] = m.fine_bytes(keys)
        set_bits = np.flatnonzero(m.bytes_to_bits(plane))
        counts, first, keys = m.share_model(sp, [b])
        assert np.array_equal(np.bincount(set_bits >> 16, minlength=512), counts)
        assert np.array_equal(set_bits & 0xFFFF, keys)
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)]))
        cut = m.share_cut(sp, [b], len(keys) // 2)
        assert sum(len(k) for k in cut.values()) == len(keys) // 2
        assert np.array_equal(np.concatenate([cut[f] for f in sorted(cut)]), keys[:len(keys) // 2])
