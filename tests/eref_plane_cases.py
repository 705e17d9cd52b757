"""The arithmetic of the count-table exchange (csrc/eref_table.hip, the end of csrc/eref_index.hip) as a numpy model, and the planted
inputs its tests use.  Not a test module: tests/test_host_eref_plane_model.py checks the model against a second statement on a CPU,
tests/test_gpu_eref_exchange_math.py checks the kernels against the model through the C ABI.  Everything here is exact.

Bit layout of a plane: key k is bit k & 31 of little-endian u32 word k >> 5 -- as bytes, np.packbits(..., bitorder="little").  The
unary planes of a count array c (values 0..3) are c >= 1, c >= 2, c >= 3.
Entry counts: entry n is the 2-bit field at bits 2n, 2n + 1 of the little-endian byte stream (eight entries per u16); hit bit n (same
bit layout as a plane) is set iff the parts' counts of entry n add up to 3 or more."""
import functools

import numpy as np

PLANE_BYTES = 1 << 29                   # 2^32 keys, one bit each
FINE_KEYS = 1 << 16                     # a fine bucket: 8 KiB of a plane
FINE_BYTES = FINE_KEYS // 8
FINE_PER_L1 = 512                       # fine buckets per level-1 bucket (key >> 25, 128 of them)
N_FINE = 1 << 16
GRID_PASS_BYTES = 2048 * 256 * 16       # what one pass of the merge / pack_low / entry-sum grids covers: 8 MiB
TRUTH_KEYS = 1 << 16                    # the truth-table slice: 8 KiB of a plane, 16 KiB of a count block
TRUTH_PLANE_BYTES = TRUTH_KEYS // 8
TRUTH_ENTRY_BYTES = TRUTH_KEYS // 4


# ---- bits and planes ------------------------------------------------------------------------------------------------------------
def bits_to_bytes(bits) -> np.ndarray:
    return np.packbits(np.asarray(bits, dtype=bool), bitorder="little")


def bytes_to_bits(data) -> np.ndarray:
    return np.unpackbits(np.asarray(data, dtype=np.uint8), bitorder="little")


def planes_of_counts(c) -> np.ndarray:
    """counts (n, a multiple of 8) -> uint8 [3][n / 8]: the planes count >= 1, >= 2, >= 3"""
    c = np.asarray(c)
    return np.stack([bits_to_bytes(c >= t) for t in (1, 2, 3)])


def counts_of_planes(planes) -> np.ndarray:
    """the reverse; the planes need not be unary (a bit of plane t simply adds one)"""
    return bytes_to_bits(planes[0]) + bytes_to_bits(planes[1]) + bytes_to_bits(planes[2])


def popcount(data) -> int:
    return int(bytes_to_bits(data).sum(dtype=np.int64))


# ---- merges ---------------------------------------------------------------------------------------------------------------------
def merge_counts(parts) -> np.ndarray:
    """parts: counts [n_parts][n] -> min(3, sum of the parts' counts) per key"""
    return np.minimum(3, np.asarray(parts).sum(axis=0, dtype=np.uint16)).astype(np.uint8)


def unary_parts(parts) -> np.ndarray:
    """counts [n_parts][n] -> the bytes merge_slices takes: [3][n_parts][n / 8]"""
    return np.ascontiguousarray(np.stack([planes_of_counts(c) for c in parts], axis=1))


def packed_parts(parts) -> np.ndarray:
    """counts [n_parts][n] -> the bytes merge_slices_packed takes: [2][n_parts][n / 8] = (low bit c & 1, high bit c >= 2)"""
    parts = np.asarray(parts)
    return np.ascontiguousarray(np.stack([np.stack([bits_to_bytes(c & 1) for c in parts]), np.stack([bits_to_bytes(c >= 2) for c in parts])]))


def low_plane(planes) -> np.ndarray:
    """pack_low: the low bit of every key's count, p1 ^ p2 ^ p3"""
    return planes[0] ^ planes[1] ^ planes[2]


# ---- entry counts ---------------------------------------------------------------------------------------------------------------
def entry_bytes(c) -> np.ndarray:
    """counts of entries (n, a multiple of 4, values 0..3) -> the count block's bytes: four entries per byte, entry n at bits 2n, 2n + 1"""
    c = np.asarray(c, dtype=np.uint8).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 2) | (c[:, 2] << 4) | (c[:, 3] << 6)).astype(np.uint8)


def entries_of_bytes(data) -> np.ndarray:
    d = np.asarray(data, dtype=np.uint8)
    return np.stack([(d >> s) & 3 for s in (0, 2, 4, 6)], axis=-1).reshape(d.shape[:-1] + (-1,))


def entry_hits(parts) -> np.ndarray:
    """parts: counts of entries [n_parts][n] -> the hit bytes: bit n set iff the parts' counts of entry n add up to 3 or more"""
    return bits_to_bytes(np.asarray(parts).sum(axis=0, dtype=np.uint16) >= 3)


# ---- the truth-table slice ------------------------------------------------------------------------------------------------------
def truth_parts(n_parts: int) -> np.ndarray:
    """[n_parts][65536]: part p gives key (or entry) k the count (k >> 2p) & 3 -- for n_parts = W <= 8 every one of the 4^W
    combinations of the parts' counts occurs, 4^(8 - W) times each"""
    assert 1 <= n_parts <= 8
    k = np.arange(TRUTH_KEYS, dtype=np.uint32)
    return np.stack([((k >> (2 * p)) & 3).astype(np.uint8) for p in range(n_parts)])


def combination_histogram(parts) -> np.ndarray:
    """how often each combination of the parts' counts occurs: 4^n_parts bins"""
    parts = np.asarray(parts, dtype=np.int64)
    code = sum(parts[p] << (2 * p) for p in range(len(parts)))
    return np.bincount(code, minlength=4 ** len(parts))


def random_counts(rng, n_parts: int, n: int) -> np.ndarray:
    return rng.integers(0, 4, size=(n_parts, n), dtype=np.uint8)


def nonzero_planes(rng, nbytes: int) -> np.ndarray:
    """uint8 [3][nbytes]: unary planes of random counts 1..3 (no key is zero) -- what a merge has to REPLACE"""
    x = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    z = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
    return np.stack([np.full(nbytes, 0xFF, np.uint8), x, x & z])


@functools.lru_cache(maxsize=None)
def long_merge_case():
    """the long merge: two parts of random counts over 8 MiB + 16 * 257 bytes of a plane -- one pass of the 2048 x 256-thread grid and
    a second, short one that is no whole number of blocks.  -> (counts [2][n] read-only, merged planes [3][bytes])"""
    rng = np.random.default_rng(8_257)
    nbytes = GRID_PASS_BYTES + 16 * 257
    parts = random_counts(rng, 2, nbytes * 8)
    parts.setflags(write=False)
    merged = planes_of_counts(merge_counts(parts))
    merged.setflags(write=False)
    return parts, merged


# ---- the sparse form of the ">= 3" plane ----------------------------------------------------------------------------------------
L1_EDGE = 37                            # the level-1 buckets 37 | 38 meet between fine buckets 37 * 512 + 511 and 38 * 512
FULL_FINE = (FINE_PER_L1 - 1, N_FINE - FINE_PER_L1)               # every bit set: the last fine bucket of level-1 bucket 0, the first of 127
ONLY_FIRST_FINE = (0, L1_EDGE * FINE_PER_L1 + FINE_PER_L1 - 1)    # only offset 0: the plane's first fine bucket, the last of a level-1 bucket
ONLY_LAST_FINE = (N_FINE - 1, (L1_EDGE + 1) * FINE_PER_L1)        # only offset 0xFFFF: the plane's last fine bucket, the first of the next level-1 bucket
LANE_EDGE_FINE = (FINE_PER_L1, 64 * FINE_PER_L1 + 5)              # offsets 255 | 256 and 16383 | 16384: a thread's and a wave's edge of the pack kernel
LANE_EDGE_OFFSETS = (255, 256, 16383, 16384)
N_RANDOM_FINE = 300


@functools.lru_cache(maxsize=None)
def sparse_plane() -> dict:
    """the planted '>= 3' plane: fine bucket -> its set bits as ascending uint16 offsets (read-only arrays)"""
    rng = np.random.default_rng(65_536)
    out = {}
    for f in FULL_FINE:
        out[f] = np.arange(FINE_KEYS, dtype=np.uint16)
    for f in ONLY_FIRST_FINE:
        out[f] = np.array([0], np.uint16)
    for f in ONLY_LAST_FINE:
        out[f] = np.array([0xFFFF], np.uint16)
    for f in LANE_EDGE_FINE:
        out[f] = np.array(LANE_EDGE_OFFSETS, np.uint16)
    # random ones: some in level-1 buckets 0 and 127 (shares of their own in the tests), the rest anywhere
    free = lambda lo, hi, n: [int(f) for f in rng.permutation(np.arange(lo, hi)) if int(f) not in out][:n]
    for f in free(0, FINE_PER_L1, 30) + free(N_FINE - FINE_PER_L1, N_FINE, 30) + free(0, N_FINE, N_RANDOM_FINE - 60):
        if f not in out:
            out[f] = np.sort(rng.choice(FINE_KEYS, size=int(rng.integers(1, 200)), replace=False)).astype(np.uint16)
    for v in out.values():
        v.setflags(write=False)
    return out


def fine_bytes(offsets) -> np.ndarray:
    """the 8 KiB of a fine bucket with these bits set"""
    bits = np.zeros(FINE_KEYS, dtype=bool)
    bits[np.asarray(offsets, dtype=np.int64)] = True
    return bits_to_bytes(bits)


def share_fine_buckets(buckets) -> np.ndarray:
    """slot -> fine bucket for a share of level-1 buckets: the buckets ascending, 512 fine buckets each"""
    return np.concatenate([np.arange(b * FINE_PER_L1, (b + 1) * FINE_PER_L1) for b in sorted(buckets)])


def share_model(sparse: dict, buckets):
    """what plane_pack leaves for a share: counts uint32 [n], first uint64 [n + 1] (exclusive prefix, first[n] = total), keys uint16 [total]"""
    fine = share_fine_buckets(buckets)
    counts = np.array([len(sparse.get(int(f), ())) for f in fine], dtype=np.uint32)
    first = np.concatenate([[0], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64)
    keys = [sparse[int(f)] for f in fine if int(f) in sparse]
    return counts, first, (np.concatenate(keys) if keys else np.zeros(0, np.uint16)).astype(np.uint16)


def share_cut(sparse: dict, buckets, cap_keys: int) -> dict:
    """the share's fine buckets as a receiver rebuilds them from a key buffer of cap_keys: only the keys inside the room"""
    counts, first, keys = share_model(sparse, buckets)
    out = {}
    for slot, f in enumerate(share_fine_buckets(buckets)):
        a, e = min(int(first[slot]), cap_keys), min(int(first[slot + 1]), cap_keys)
        out[int(f)] = keys[a:e]
    return out
