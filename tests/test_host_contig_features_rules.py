"""The feature rules of phage_scoring as tests/contig_feature_cases.py restates them, against what the reference's
compiled encode.matrix_encoding returned (tests/golden/contig_features_cases.npz)."""
import os

import numpy as np
import pytest

from tests import contig_feature_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contig_features_cases.npz")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return [(z["seq_%02d" % k].tobytes(), z["feat_%02d" % k]) for k in range(int(z["n"]))]


def test_golden_holds_the_seeded_sequences(golden):
    assert [s for s, _ in golden] == cc.golden_sequences()
    assert len(golden) == len(cc.GOLDEN_LENGTHS) and {len(s) for s, _ in golden} == set(cc.GOLDEN_LENGTHS)


def test_restatement_equals_the_reference_bit_for_bit(golden):
    for seq, want in golden:
        got = cc.reference_features(seq)
        assert got.dtype == np.float64 and got.shape == (cc.CELLS,)
        assert got.tobytes() == want.tobytes(), len(seq)


def test_model_layout_is_the_moveaxis_of_the_reference(golden):
    for seq, want in golden:
        feat, _ = cc.model_features(seq)
        moved = np.moveaxis(want.reshape(3, 4096), 0, 1).reshape(-1).astype(np.float32)
        assert feat.tobytes() == moved.tobytes(), len(seq)


def test_fsum_from_integer_row_sums_is_within_one_ulp(golden):
    worst = 0.0
    for seq, want in golden:
        _, fsum = cc.model_features(seq)
        ref = cc.reference_fsum(want)
        ulp = np.spacing(np.maximum(np.abs(ref), np.abs(fsum)))
        worst = max(worst, float(np.max(np.abs(fsum.astype(np.float64) - ref.astype(np.float64)) / ulp)))
    print("fsum: worst distance in float32 ulps", worst)
    assert worst <= 1.0


@pytest.mark.parametrize("m, first, total", [(5, 0, 0), (6, 1, 1), (7, 2, 3), (8, 3, 6)])
def test_thresholds(m, first, total):
    """m - 5 - d pairs per distance: the first matrix holds 0, 1, 2, 3 non-zero cells at m = 5, 6, 7, 8, the three together
    0, 1, 2 + 1, 3 + 2 + 1"""
    seq = b"ACGTTGCA"[:m]                                # no pair of 3-mers occurs twice
    c, got_m = cc.counts(seq)
    assert got_m == m
    assert int((c[0] != 0).sum()) == first and int((c != 0).sum()) == total == int(c.sum())
    assert [int(c[d].sum()) for d in range(3)] == [max(m - 5 - d, 0) for d in range(3)]


def test_dropped_bytes_are_spanned_and_still_counted_in_the_length():
    a, m = cc.counts(b"ACGTTGCATC")
    b, mb = cc.counts(b"AC-GTnTGCA*TC")
    assert m == mb == 10 and (a == b).all() and a.max() == 1
    assert cc.reference_features(b"AC-GTnTGCA*TC").max() == 1 / 13 * 100


def test_empty_sequence_gives_nan():
    feat, fsum = cc.model_features(b"")
    assert np.isnan(feat).all() and np.isnan(fsum).all()
