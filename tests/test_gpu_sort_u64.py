"""palace_sort_u64 (palace_amd/csrc/bam_sort.hip) through the C ABI against numpy.argsort(kind="stable") of the keys' low key_bits
bits: the sizes around a wave, around the tile T of one workgroup and beyond two tiles; key sets that put everything into one digit,
into two, into the top byte or the bottom bit only; random keys at key_bits that end inside, on and between the 8-bit passes; and
bits above key_bits set to garbage, which the header says are ignored."""
import numpy as np
import pytest

from palace_amd import capi

pytestmark = pytest.mark.gpu

T = capi.SORT_TILE
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 200003]


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx() as c:
        yield c


def check(ctx, keys, key_bits):
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out, perm = capi.sort_u64(ctx, keys, key_bits)
    low = keys if key_bits == 64 else keys & np.uint64((1 << key_bits) - 1)
    want = np.argsort(low, kind="stable")
    assert np.array_equal(perm, want.astype(np.uint32)), (len(keys), key_bits)
    assert np.array_equal(out, keys[want])


@pytest.mark.parametrize("n", SIZES)
def test_fixed_key_sets(ctx, n):
    idx = np.arange(n, dtype=np.uint64)
    check(ctx, np.full(n, 0x0123456789abcdef, np.uint64), 64)               # all equal: the permutation is the identity
    out, perm = capi.sort_u64(ctx, np.full(n, 7, np.uint64), 64)
    assert np.array_equal(perm, np.arange(n, dtype=np.uint32))
    check(ctx, np.where(idx % np.uint64(3) == 0, np.uint64(5 << 40), np.uint64(9)), 64)        # two distinct values
    check(ctx, np.uint64(1 << 52) - idx, 53)                                 # strictly descending
    check(ctx, (idx * np.uint64(2654435761) % np.uint64(256)) << np.uint64(56), 64)            # only the top byte differs
    check(ctx, (idx * np.uint64(2654435761) >> np.uint64(7)) & np.uint64(1) | np.uint64(0xabcdef00), 64)  # only the bottom bit differs
    check(ctx, idx, 0)                                                       # no key bits: the input order


@pytest.mark.parametrize("n", SIZES)
def test_random_keys(ctx, n):
    rng = np.random.default_rng(1000 + n)
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    for key_bits in (1, 8, 9, 53, 64):
        tight = keys if key_bits == 64 else keys & np.uint64((1 << key_bits) - 1)
        check(ctx, tight, key_bits)                                          # nothing above key_bits
        check(ctx, keys, key_bits)                                           # garbage above key_bits: ignored
    few = rng.integers(0, 40, n, dtype=np.uint64)                            # many equal keys: stability among them
    check(ctx, few | (rng.integers(0, 1 << 20, n, dtype=np.uint64) << np.uint64(9)), 9)
    check(ctx, few << np.uint64(33), 53)


def test_result_does_not_depend_on_key_bits_being_tight(ctx):
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 1 << 20, 3 * T + 17, dtype=np.uint64)
    a = capi.sort_u64(ctx, keys, 20)
    for key_bits in (21, 24, 25, 40, 64):
        b = capi.sort_u64(ctx, keys, key_bits)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
