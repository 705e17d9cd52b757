"""palace_bgzf_deflate_lz at the C ABI (csrc/bgzf_deflate.hip, csrc/deflate_lz.hpp), on caller-owned buffers with guards:

* the catalogue of tests/deflate_lz_cases.py as one batch per text misalignment 0 .. 3: every member is byte-identical to the member
  the CPU build of the same headers writes (which tests/test_host_deflate_lz.py holds to the exact model) -- the head table's atomic
  max, the distances in device memory, the workgroup scan and the merge give what a thread-by-thread run gives;
* the slot in front of the batch, the slot behind it and every slot's bytes behind its member keep the guard fill;
* about 700 short distinct pieces in one launch -- more members than workgroups, so every workgroup takes several, one after the
  other in the same LDS -- give, member for member, what each gives in a launch of its own;
* palace_bgzf_compact and palace_bgzf_inflate take the batch round;
* two runs give the same bytes."""
import os
import zlib

import numpy as np
import pytest

from palace_amd import capi
from tests import deflate_enc_checks as ck
from tests import deflate_lz_cases as lc

pytestmark = pytest.mark.gpu

FILL = 0xa5
TOOL = os.path.join(ck.ROOT, "palace_amd", "bin", "deflate_lz_selftest")
LARGEST = 18 + 5 + lc.MAX_TEXT + 8


def deflate(ctx, pieces, lead, before=1, after=1):
    """-> (member lengths, every slot) of one launch over `pieces`, the first one `lead` bytes into the text buffer"""
    lens = np.array([len(p) for p in pieces], np.int64)
    offs = lead + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return capi.bgzf_deflate_slots(ctx, bytes(lead) + b"".join(pieces), offs, lens, [zlib.crc32(p) for p in pieces], before=before, after=after,
                                   fill=FILL, lz=True)


def members_of(mlen, slots, first=1):
    return [slots[first + k, :int(n)].tobytes() for k, n in enumerate(mlen)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    ck.make(TOOL)
    return ck.host_members(tmp_path_factory.mktemp("lz_gpu"), [p for _, p in lc.cases()], 0, tool=TOOL)


@pytest.fixture(scope="module")
def device():
    pieces = [p for _, p in lc.cases()]
    runs = []
    with capi.Ctx(0) as ctx:
        for lead in (0, 1, 2, 3, 0):                                       # (lead 0 twice: the same bytes both times)
            mlen, slots = deflate(ctx, pieces, lead)
            assert ((mlen >= 28) & (mlen <= LARGEST)).all(), mlen
            spilled = [lc.cases()[k][0] for k, n in enumerate(mlen) if not (slots[1 + k, (int(n) + 3) & ~3:] == FILL).all()]
            runs.append((members_of(mlen, slots), bool((slots[0] == FILL).all() and (slots[-1] == FILL).all()), spilled))
    return runs


@pytest.mark.parametrize("lead", range(4))
def test_every_member_is_the_cpu_builds_member(host, device, lead):
    members, guards_intact, spilled = device[lead]
    differ = [(name, len(a), len(b)) for (name, _), a, b in zip(lc.cases(), members, host) if a != b]
    assert not differ, (len(differ), differ[:10])
    assert guards_intact, "the slot in front of the batch or the one behind it changed"
    assert not spilled, ("bytes changed behind the member in the slots of", spilled[:10])
    assert all(len(m) <= len(p) + 31 for (_, p), m in zip(lc.cases(), members))


def test_two_runs_give_the_same_bytes(device):
    assert device[0][0] == device[4][0]


def short_pieces(n=700):
    """distinct texts of 1 to 3000 bytes with repeats a few rounds back, a few of them empty"""
    rng = np.random.default_rng(700)
    out = []
    for k in range(n):
        if k % 97 == 50:
            out.append(b"")
            continue
        size = int(rng.integers(1, 3001))
        unit = rng.integers(0, int(rng.integers(2, 200)), int(rng.integers(5, 700)), dtype=np.uint8).tobytes()
        text = bytearray((unit * (size // len(unit) + 1))[:size])
        for at in rng.integers(0, size, size // 50):
            text[int(at)] = int(rng.integers(0, 256))
        out.append(b"%d:" % k + bytes(text))
    assert len({p for p in out if p}) == n - sum(1 for p in out if not p)
    return out


def test_a_batch_gives_what_every_piece_gives_alone_and_round_trips():
    pieces = short_pieces()
    with capi.Ctx(0) as ctx:
        mlen, slots = deflate(ctx, pieces, 1)
        batch = members_of(mlen, slots)
        assert (slots[0] == FILL).all() and (slots[-1] == FILL).all()
        alone = []
        for p in pieces:
            n1, s1 = deflate(ctx, [p], 1, before=0, after=0)
            alone.append(s1[0, :int(n1[0])].tobytes())
        file, moff = capi.bgzf_deflate(ctx, pieces, lead=3, lz=True)
        full = [k for k, p in enumerate(pieces) if p]                       # (the EOF member holds no text to hand to the inflater)
        st, inflated = capi.bgzf_inflate_members(ctx, [batch[k] for k in full], [len(pieces[k]) for k in full])
    differ = [k for k, (a, b) in enumerate(zip(batch, alone)) if a != b]
    assert not differ, (len(differ), differ[:10])
    assert sum(1 for m in batch if m[18] & 6 == 4) > 300                    # BTYPE 10: most of them are coded, with matches to leak
    assert [zlib.decompress(m, 31) for m in batch] == pieces
    # the compaction: the members one behind the other at exact offsets
    assert moff[-1] == len(file) and file == b"".join(batch) and list(np.diff(moff)) == [len(m) for m in batch]
    assert (st == 0).all(), np.flatnonzero(st)[:10]
    assert inflated == [pieces[k] for k in full]
