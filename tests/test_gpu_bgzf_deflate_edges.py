"""palace_bgzf_deflate and palace_bgzf_compact at the C ABI (csrc/bgzf_deflate.hip), on caller-owned buffers with guards:

* the edge catalogue of tests/deflate_enc_cases.py as one batch per text misalignment 0 .. 3: every member is byte-identical to the
  member the CPU build of the same header writes (tests/test_host_deflate_enc_edges.py) -- "the output is a function of the input
  alone" held across builds, which is what a fault in the workgroup scan, the LDS atomics or the merge would break -- passes the
  reader and model checks of tests/deflate_enc_checks.py, and inflates to its piece in palace_bgzf_inflate;
* a member alone between two spare slots, for the largest members, d_len = -1 and d_len = 0xff01: nothing outside its slot changes;
* palace_bgzf_compact on synthetic slots, no encoder involved, up to 2049 members (the scan carries a sum across rounds of 1024):
  exact 64-bit prefix sums, the file bytes, and not a byte in front of the base or behind the total."""
import zlib

import numpy as np
import pytest

from palace_amd import capi
from tests import deflate_enc_cases as dc
from tests import deflate_enc_checks as ck
from tests import tabix_reader as tr

pytestmark = pytest.mark.gpu

SLOT = capi.BGZF_SLOT
FILL = 0xa5
LARGEST = 18 + 5 + dc.MAX_TEXT + 8                                       # a stored member of 0xff00 bytes: 65311


def deflate(ctx, pieces, lead):
    """-> (members, every slot) of one launch over `pieces`, the first one `lead` bytes into the text buffer"""
    lens = np.array([len(p) for p in pieces], np.int64)
    offs = lead + np.concatenate([[0], np.cumsum(lens)[:-1]])
    mlen, slots = capi.bgzf_deflate_slots(ctx, bytes(lead) + b"".join(pieces), offs, lens, [zlib.crc32(p) for p in pieces], fill=FILL)
    return mlen, slots


def rest_untouched(slot, member_len):
    """The slot still holds the fill behind the dword of the member's last byte.  The header calls those bytes undefined, so the
    member's own workgroup may write them; the writer as it stands never does, and while that is so a changed byte there can only
    be a neighbour's that left its slot -- which the spare slots around a batch cannot see for the members in its middle."""
    return bool((slot[(member_len + 3) & ~3:] == FILL).all())


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    ck.make(ck.TOOL)
    return ck.host_members(tmp_path_factory.mktemp("enc_edges_gpu"), [p for _, p in dc.cases()], 0)


@pytest.fixture(scope="module")
def device():
    """per lead: (members, first and last spare slot untouched, the pieces behind whose member the slot changed); and the device inflater's verdict on the members of lead 0"""
    pieces = [p for _, p in dc.cases()]
    runs = []
    with capi.Ctx(0) as ctx:
        for lead in range(4):
            mlen, slots = deflate(ctx, pieces, lead)
            assert ((mlen >= 28) & (mlen <= LARGEST)).all(), mlen[(mlen < 28) | (mlen > LARGEST)][:10]
            spilled = [dc.cases()[k][0] for k, n in enumerate(mlen) if not rest_untouched(slots[1 + k], int(n))]
            runs.append(([slots[1 + k, :int(n)].tobytes() for k, n in enumerate(mlen)], bool((slots[0] == FILL).all() and (slots[-1] == FILL).all()),
                         spilled))
        st, inflated = capi.bgzf_inflate_members(ctx, runs[0][0], [len(p) for p in pieces])
    return dict(runs=runs, st=st, inflated=inflated)


@pytest.mark.parametrize("lead", range(4))
def test_every_member_is_the_cpu_builds_member(host, device, lead):
    members, spare_untouched, spilled = device["runs"][lead]
    differ = [(name, len(a), len(b)) for (name, _), a, b in zip(dc.cases(), members, host) if a != b]
    assert not differ, (len(differ), differ[:10])
    assert spare_untouched, "the slot in front of the batch or the one behind it changed"
    assert not spilled, ("bytes changed behind the member in the slots of", len(spilled), spilled[:10])


@pytest.mark.parametrize("lead", range(4))
def test_every_member_is_what_the_model_says(device, lead):
    named = dc.cases()
    faults, btype = ck.catalogue_faults(named, device["runs"][lead][0])
    assert not faults, (len(faults), faults[:20])
    assert len(btype) == len(named) and all(btype[n] in (0, 2) for n, p in named if p)


def test_the_device_inflater_reads_every_member(device):
    assert (device["st"] == 0).all(), [n for (n, _), s in zip(dc.cases(), device["st"]) if s][:10]
    wrong = [name for (name, piece), got in zip(dc.cases(), device["inflated"]) if got != piece]
    assert not wrong, wrong[:10]


def alone(ctx, blob, off, length, crc):
    """one member between two spare slots -> (member, nothing outside its slot changed)"""
    mlen, slots = capi.bgzf_deflate_slots(ctx, blob, [off], [length], [crc], before=1, after=1, fill=FILL)
    return slots[1, :int(mlen[0])].tobytes(), bool((slots[0] == FILL).all() and (slots[2] == FILL).all() and rest_untouched(slots[1], int(mlen[0])))


def test_a_member_alone_stays_in_its_slot(host):
    by = {name: (piece, m) for (name, piece), m in zip(dc.cases(), host)}
    names = [f"size_{n}_{kind}" for n in (0xfeff, 0xff00) for kind in ("no_lf", "all_lf", "lf_first", "lf_last", "short_lines")]
    names += ["piece_random", "piece_newlines", "piece_fibonacci", "distance_32768", f"distance_{dc.TOO_FAR}_no_match", "size_1_no_lf", "size_513_short_lines"]
    assert len(by["piece_random"][1]) == LARGEST
    with capi.Ctx(0) as ctx:
        for k, name in enumerate(names):
            piece, want = by[name]
            got, inside = alone(ctx, bytes(k % 4) + piece, k % 4, len(piece), zlib.crc32(piece))
            assert got == want, name
            assert inside, name


def test_lengths_outside_the_range_are_the_nearest_member():
    """d_len = -1 is an empty piece: the EOF member; d_len = 0xff01 is cut to 0xff00 bytes: at most 65311 bytes of member"""
    rng = np.random.default_rng(8)
    noise = rng.integers(0, 256, dc.MAX_TEXT + 64, dtype=np.uint8).tobytes()
    lines = (b"NODE_1_length_70000_cov_3.5\t12345\t17\n" * 1800)[:dc.MAX_TEXT + 64]
    with capi.Ctx(0) as ctx:
        got, inside = alone(ctx, noise, 2, -1, 0)
        assert got == tr.EOF_MEMBER and inside
        for text, lead in ((noise, 1), (lines, 3)):
            piece = text[lead:lead + dc.MAX_TEXT]
            got, inside = alone(ctx, text, lead, 0xff01, zlib.crc32(piece))
            assert inside and len(got) <= LARGEST
            faults, kind, _, _ = ck.member_faults(piece, got)
            assert not faults and kind == (0 if text is noise else 2), faults


# ---- palace_bgzf_compact on synthetic slots ---------------------------------------------------------------------------------------

COUNTS = [0, 1, 2, 1023, 1024, 1025, 2048, 2049]


def member_lengths(n, seed):
    """from the EOF member's 28 bytes and the three lengths behind it (every phase of a dword) to the largest member, and between"""
    rng = np.random.default_rng(seed)
    kind = rng.random(n)
    out = np.where(kind < 0.6, rng.integers(28, 32, n), np.where(kind < 0.7, LARGEST, rng.integers(28, LARGEST + 1, n)))
    if n >= 2:
        out[0], out[-1] = LARGEST, 29
    return out.astype(np.int32)


@pytest.fixture(scope="module")
def slots():
    """2049 slots of bytes that tell their slot and their place in it, on the host and on the device"""
    n = max(COUNTS)
    at = np.arange(SLOT, dtype=np.uint32)
    host = (at * 131 + (at >> 8) * 7).astype(np.uint8)[None, :] + (np.arange(n, dtype=np.uint32) * 89).astype(np.uint8)[:, None]
    assert host.dtype == np.uint8 and host.shape == (n, SLOT)
    with capi.Ctx(0) as ctx:
        d = ctx.upload(host.reshape(-1))
        yield ctx, d, host
        d.free()


@pytest.mark.parametrize("n", COUNTS)
def test_compaction_is_the_concatenation_at_exact_offsets(slots, n):
    ctx, d_slots, host = slots
    lens = member_lengths(n, 100 + n)
    want_off = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
    want = np.concatenate([host[m, :lens[m]] for m in range(n)]) if n else np.zeros(0, np.uint8)
    total = int(want_off[-1])
    assert len(want) == total
    for base in range(4):
        moff, buf = capi.bgzf_compact_slots(ctx, d_slots, lens, base=base, fill=0x5a, room=64)
        assert moff.dtype == np.int64 and np.array_equal(moff, want_off), (n, base, np.flatnonzero(moff != want_off)[:5])
        assert np.array_equal(buf[base:base + total], want), (n, base, np.flatnonzero(buf[base:base + total] != want)[:5])
        assert (buf[:base] == 0x5a).all() and (buf[base + total:] == 0x5a).all() and len(buf) == base + total + 64, (n, base)
