"""palace_bam_sort_keys, palace_bam_gather_plan and palace_bam_gather_write (palace_amd/csrc/bam_sort.hip) through the C ABI on
inflated streams built here from record encodings -- no BGZF involved.  Expectations come from the Python restatement of
tests/bam_sort_cases.py (the key of DESIGN.md section 8, Python's stable sort), never from the device."""
import random

import numpy as np
import pytest

from palace_amd import capi
from tests import bam_sort_cases as bc
from tests.test_host_bam_spec import aux_Z, record

pytestmark = pytest.mark.gpu

HEAD = bytes(range(101))                    # a stand-in for the header; its odd length puts the records at no alignment


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx() as c:
        yield c


def starts_of(recs, first):
    out, p = [], first
    for r in recs:
        out.append(p + 4)
        p += len(r)
    return np.array(out, dtype=np.int64)


def sort_on_device(ctx, recs, n_ref, new_head=b"\x42" * 77):
    """keys -> sort -> plan -> write; checked against the restatement at every step"""
    stream = HEAD + b"".join(recs)
    starts = starts_of(recs, len(HEAD))
    keys, n_bad, first_bad = capi.bam_sort_keys(ctx, stream, starts, n_ref)
    assert (n_bad, first_bad) == (0, -1)
    assert keys.tolist() == [bc.sort_key(r, n_ref) for r in recs]
    out_keys, perm = capi.sort_u64(ctx, keys, 33 + int(n_ref).bit_length())
    order = sorted(range(len(recs)), key=lambda k: bc.sort_key(recs[k], n_ref))
    assert perm.tolist() == order
    off, new_starts, image = capi.bam_gather(ctx, stream, starts, perm, new_head)
    want = bc.sorted_records(recs, n_ref)
    want_off = np.cumsum([len(new_head)] + [len(r) for r in want])
    assert off.tolist() == want_off.tolist() and new_starts.tolist() == (want_off[:-1] + 4).tolist()
    assert image == new_head + b"".join(want) + b"\xaa" * 16                # every byte, and nothing outside [off[0], off[n])
    return want


def test_keys_and_bad_records(ctx):
    n_ref = 50
    recs = [record("a", 0, 3, 100, 60, "10M"), record("b", 16, 3, 100, 60, "10M"), record("c", 0, 3, -1, 0, "10M"), record("d", 4, -1, -1, 0, "", l_seq=3),
            record("e", 4, -1, 500, 0, "", l_seq=3), record("f", 0, 49, 0x7ffffffe, 0, "1M"), record("g", 0, 0, 0, 0, "1M")]
    stream = HEAD + b"".join(recs)
    keys, n_bad, first_bad = capi.bam_sort_keys(ctx, stream, starts_of(recs, len(HEAD)), n_ref)
    assert (n_bad, first_bad) == (0, -1) and keys.tolist() == [bc.sort_key(r, n_ref) for r in recs]
    assert keys[0] + 1 == keys[1] and keys[2] < keys[0] and keys[3] >> 33 == n_ref and keys[6] == 2
    bad = recs[:2] + [record("x", 0, n_ref, 5, 0, "1M")] + recs[2:5] + [record("y", 0, -2, 5, 0, "1M"), record("z", 0, 1, -2, 0, "1M")] + recs[5:]
    _, n_bad, first_bad = capi.bam_sort_keys(ctx, HEAD + b"".join(bad), starts_of(bad, len(HEAD)), n_ref)
    assert (n_bad, first_bad) == (3, 2)
    assert [k for k, r in enumerate(bad) if not bc.key_ok(r, n_ref)] == [2, 6, 7]


def test_no_record_and_one_record(ctx):
    assert sort_on_device(ctx, [], 5) == []
    sort_on_device(ctx, [record("only", 16, 2, 77, 60, "30M")], 5)
    sort_on_device(ctx, [record("only", 16, 2, 77, 60, "30M")], 5, new_head=b"")


def test_every_record_equal_keyed(ctx):
    recs = [record(f"r{k}", 0, 1, 1000, k % 60, f"{10 + k % 7}M", aux=aux_Z("XS", "q" * (k % 11))) for k in range(3000)]
    assert sort_on_device(ctx, recs, 4) == recs                              # stable: the input order


def test_one_reference_and_seventy_thousand(ctx):
    rng = random.Random(7)
    sort_on_device(ctx, bc.random_records(rng, 3000, [("only", 100000)]), 1)
    n_ref = 70000                                                           # refID needs more than 16 bits
    recs = [record(f"r{k}", 16 * (k & 1), rng.choice((0, 1, 65535, 65536, 65537, 69999, rng.randrange(n_ref))), rng.randrange(500), 60, "20M")
            for k in range(4000)] + [record("u", 4, -1, -1, 0, "", l_seq=1)]
    rng.shuffle(recs)
    sort_on_device(ctx, recs, n_ref)


def test_a_long_record_among_short_ones(ctx):
    rng = random.Random(8)
    recs = bc.random_records(rng, 400, [("a", 5000), ("b", 900)])
    big = record("big", 0, 0, 2500, 60, "100M", aux=aux_Z("XL", "L" * 200000))
    assert len(big) >= 200000
    recs.insert(137, big)
    sort_on_device(ctx, recs, 2)


def test_the_smallest_records_share_a_lane(ctx):
    rng = random.Random(9)
    recs = [record("n" * rng.randrange(0, 4), 4 | 16 * rng.randrange(2), rng.choice((-1, 0, 1)), rng.randrange(-1, 30), 0, "", l_seq=0) for _ in range(5000)]
    assert {len(r) for r in recs} == {37, 38, 39, 40}
    sort_on_device(ctx, recs, 2)


def test_random_records(ctx):
    rng = random.Random(10)
    targets = [("a", 1 << 29), ("b", 5000), ("c", 300000), ("d", 70000), ("e", 40)]
    recs = bc.random_records(rng, 20000, targets)
    sort_on_device(ctx, recs, len(targets))
