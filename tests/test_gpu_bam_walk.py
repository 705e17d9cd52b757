"""palace_bam_walk and palace_bam_match_segments (palace_amd/csrc/bam.hip) through the C ABI, on inflated streams built here from
record encodings -- no BGZF involved.  Expectations come from the serial restatement below: BamLoad::walk_step and the
match-segment rules of decode_range (palace_amd/host/bam.cpp), never from the device."""
import struct

import numpy as np
import pytest

from palace_amd import capi, synth
from tests.test_host_bam_spec import aux_A, aux_B, aux_i, aux_Z, cigar_words, record

pytestmark = pytest.mark.gpu

N_REF = 50
FIRST = 100                                 # a stand-in for the header: the walk never looks at it
HEAD = bytes(range(100))


# ---- the serial restatement -----------------------------------------------------------------------------------------------------
def le16(d, p): return d[p] | (d[p + 1] << 8)
def le32(d, p): return d[p] | (d[p + 1] << 8) | (d[p + 2] << 16) | (d[p + 3] << 24)
def s32(v): return v - (1 << 32) if v & 0x80000000 else v


def serial_walk(d, first):
    """-> (offset of every record's refID, offset at which the walk stopped)"""
    total, p, starts = len(d), first, []
    while p + 4 <= total:
        bs = le32(d, p)
        if bs < 32 or p + 4 + bs > total:
            break
        r = p + 4
        l_name, n_cig, l_seq = d[r + 8], le16(d, r + 12), le32(d, r + 16)
        if l_name < 1 or l_seq > 0x7fffffff or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            break
        starts.append(r)
        p += 4 + bs
    return starts, p


def aux_size(d, ty, v, end):
    ty = chr(ty)
    if ty in "AcC":
        return 1
    if ty in "sS":
        return 2
    if ty in "iIf":
        return 4
    if ty in "ZH":
        z = d.find(b"\0", v, end)
        return z - v + 1 if z >= 0 else 0
    if ty == "B":
        if end - v < 5:
            return 0
        es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(chr(d[v]), 0)
        return 5 + es * le32(d, v + 1) if es else 0
    return 0


def serial_segments(d, starts, n_ref):
    out = []
    for r in starts:
        end = r + le32(d, r - 4)
        tid, pos = s32(le32(d, r)), s32(le32(d, r + 4))
        l_name, n_cig, flag, l_seq = d[r + 8], le16(d, r + 12), le16(d, r + 14), le32(d, r + 16)
        if (flag & 0x704) or not 0 <= tid < n_ref or pos < 0:
            continue
        cg = r + 32 + l_name
        ops, n_ops = cg, n_cig
        if n_cig > 0 and le32(d, cg) & 15 == 4 and le32(d, cg) >> 4 == l_seq:
            x = cg + 4 * n_cig + (l_seq + 1) // 2 + l_seq
            while x + 3 <= end:
                v = x + 3
                sz = aux_size(d, d[x + 2], v, end)
                if not sz or sz > end - v:
                    break
                if d[x:x + 2] == b"CG":
                    if d[x + 2] == ord("B") and d[v] in b"Ii" and n_cig <= le32(d, v + 1) < (1 << 29):
                        ops, n_ops = v + 5, le32(d, v + 1)
                    break
                x = v + sz
        rl = 0
        for k in range(n_ops):
            w = le32(d, ops + 4 * k)
            op, ln = w & 15, w >> 4
            if ln > 0 and op in (0, 7, 8):
                out.append((tid, pos + rl, ln))
            if op in (0, 2, 3, 7, 8):
                rl += ln
    return out


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def plain(k, cigar="30M", tid=None, pos=None):
    return synth.BamRecord(f"p{k}", 0, k % N_REF if tid is None else tid, 10 + k if pos is None else pos, 60, cigar).encode()


def check_walk(ctx, stream, first, chunk, n_ref=N_REF):
    want, stop = serial_walk(stream, first)
    got, got_stop, stats = capi.bam_walk(ctx, stream, first, n_ref, chunk)
    assert len(got) == len(want) and got_stop == stop
    assert got.tolist() == want
    return want, stats


@pytest.fixture(scope="module")
def random_stream():
    rng = synth.rng_for(20261017)
    parts = [HEAD]
    for k in range(2000):
        ops = "".join(f"{int(rng.integers(0, 31))}{'MIDNSHP=X'[int(rng.integers(0, 9))]}" for _ in range(int(rng.integers(0, 41))))
        name = "".join(chr(int(c)) for c in rng.integers(33, 127, size=int(rng.integers(1, 255))))
        flag = [0, 0, 0, 16, 0x4, 0x100, 0x400, 0x800][int(rng.integers(0, 8))]
        parts.append(synth.BamRecord(name, flag, int(rng.integers(-1, N_REF)), int(rng.integers(-1, 100000)), 60, ops,
                                     mtid=int(rng.integers(-1, N_REF)), mpos=int(rng.integers(-1, 100000))).encode())
    stream = b"".join(parts)
    return stream, serial_walk(stream, FIRST)


# ---- the walk ---------------------------------------------------------------------------------------------------------------------
def test_hand_case(ctx):
    """three records; every offset written out: a record is 4 + 32 + l_read_name + 4 n_cigar + (l_seq + 1) / 2 + l_seq + 15 bytes of
    the writer's aux fields (AS:C 4, NM:C 4, XS:i 7)"""
    recs = [synth.BamRecord("a", 0, 0, 5, 60, "10M").encode(),       # 4 + 32 + 2 + 4 + 5 + 10 + 15 = 72
            synth.BamRecord("bcd", 0, 1, 7, 60, "3S4M").encode(),    # 4 + 32 + 4 + 8 + 4 + 7 + 15 = 74
            synth.BamRecord("ef", 4, -1, -1, 0, "").encode()]        # 4 + 32 + 3 + 0 + 0 + 0 + 15 = 54
    assert [len(r) for r in recs] == [72, 74, 54]
    stream = HEAD + b"".join(recs)
    got, stop, stats = capi.bam_walk(ctx, stream, FIRST, 2)
    assert got.tolist() == [104, 176, 250] and stop == 300 == len(stream)
    assert stats["chunks"] == 1 and stats["held"] == 1 and stats["repaired"] == 0
    tid, pos, ln = capi.bam_match_segments(ctx, stream, got, 2)
    assert (tid.tolist(), pos.tolist(), ln.tolist()) == ([0, 1], [5, 7], [10, 4])


@pytest.mark.parametrize("chunk", [256, 4096, 0])
def test_random_records(ctx, random_stream, chunk):
    stream, (want, stop) = random_stream
    assert len(want) == 2000 and stop == len(stream)
    got, got_stop, stats = capi.bam_walk(ctx, stream, FIRST, N_REF, chunk)
    assert got_stop == stop and got.tolist() == want
    assert stats["chunks"] == -(-(len(stream) - FIRST) // (chunk or 65536))
    if chunk == 256:
        assert stats["no_start"] > 0                # records of a kilobyte: most chunks hold no record start
    seg = capi.bam_match_segments(ctx, stream, got, N_REF)
    assert list(zip(*(a.tolist() for a in seg))) == serial_segments(stream, want, N_REF)


def cg_record(n_ops_half=35000):
    """a CG:B,I record as tests/test_host_bam_spec.py builds it: the real CIGAR (1M1D x 35 000 = 70 000 ops) in the tag behind the
    <l_seq>S<ref>N placeholder"""
    long_ops = cigar_words("1M1D" * n_ops_half)
    return record("r_cg", 0, 2, 7, 30, [(n_ops_half << 4) | 4, (2 * n_ops_half << 4) | 3], l_seq=n_ops_half, aux=aux_i("NM", 1) + aux_B("CG", "I", long_ops))


@pytest.mark.parametrize("chunk", [4096, 0])
def test_records_longer_than_many_chunks(ctx, chunk):
    parts = [HEAD] + [plain(k) for k in range(40)]
    parts.append(synth.BamRecord("long", 0, 1, 0, 60, "300000M").encode())          # 450 KB: seven chunks of 64 KiB
    parts += [plain(k) for k in range(40, 80)]
    parts.append(cg_record())                                                        # 280 KB of CIGAR in the tag
    parts += [plain(k) for k in range(80, 700)]
    stream = b"".join(parts)
    want, stats = check_walk(ctx, stream, FIRST, chunk)
    assert len(want) == 702 and stats["chunks"] > 8
    seg = capi.bam_match_segments(ctx, stream, want, N_REF)
    exp = serial_segments(stream, want, N_REF)
    assert list(zip(*(a.tolist() for a in seg))) == exp and len(exp) == 700 + 1 + 35000


def test_decoy_in_the_quality_bytes(ctx):
    """a record whose quality bytes hold a byte-exact copy of six valid records, beginning exactly on a chunk border: the chunk's
    guess is the copy, the chain enters the chunk behind the record and has to walk it itself"""
    chunk = 4096
    copy = b"".join(plain(900 + k, "20M") for k in range(6))
    host = bytearray(synth.BamRecord("host", 0, 3, 50, 60, "1500M").encode())
    qual_at = 4 + 32 + 5 + 4 + 750                                                   # in the record: name "host\0", one op, 750 bytes of bases
    assert bytes(host[qual_at:qual_at + 1500]) == b"\xff" * 1500 and len(copy) < 1300
    front = [plain(k) for k in range(120)]
    base = FIRST + sum(len(r) for r in front)
    fill = None                                                                      # filler records that put the border 100 bytes into the qualities
    for n200 in range(0, 25):
        for ln in range(1, 255):
            if (base + n200 * 200 + 52 + ln + qual_at + 100 - FIRST) % chunk == 0:
                fill = [synth.BamRecord("f" * 148, 4, -1, -1, 0, "").encode()] * n200 + [synth.BamRecord("g" * ln, 4, -1, -1, 0, "").encode()]
                break
        if fill:
            break
    assert fill and all(len(f) == 200 for f in fill[:-1])
    host_at = base + sum(len(f) for f in fill)
    border = host_at + qual_at + 100
    assert (border - FIRST) % chunk == 0
    host[qual_at + 100:qual_at + 100 + len(copy)] = copy
    stream = HEAD + b"".join(front + fill) + bytes(host) + b"".join(plain(k) for k in range(200, 400))
    assert stream[border:border + len(copy)] == copy and host_at + len(host) < border + chunk
    assert len(serial_walk(stream, border)[0]) == 6                                  # from the border the copy walks like records
    want, stats = check_walk(ctx, stream, FIRST, chunk)
    assert border + 4 not in want and len(want) == 120 + len(fill) + 1 + 200
    assert stats["repaired"] >= 1


def malformed(kind):
    good = bytearray(plain(7777))
    if kind == "block_size 31":
        return struct.pack("<I", 31) + bytes(good[4:4 + 31])
    if kind == "past total":
        return struct.pack("<I", 1 << 30) + bytes(good[4:])
    if kind == "l_read_name 0":
        good[4 + 8] = 0
        return bytes(good)
    if kind == "fields larger than block_size":
        good[4 + 16:4 + 20] = struct.pack("<I", 5000)                                # l_seq: bases and qualities do not fit
        return bytes(good)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["block_size 31", "past total", "l_read_name 0", "fields larger than block_size"])
@pytest.mark.parametrize("at", [2, 300])
def test_malformed_record_ends_the_stream(ctx, kind, at):
    """once in chunk 0, once several chunks in behind good guesses (300 records of 91 bytes, chunks of 4 096); good records follow"""
    recs = [plain(k) for k in range(600)]
    stream = HEAD + b"".join(recs[:at]) + malformed(kind) + b"".join(recs[at:])
    want, stats = check_walk(ctx, stream, FIRST, 4096)
    assert len(want) == at and stats["chunks"] > 10
    if at == 300:
        assert stats["held"] >= 5


def test_degenerate_streams(ctx):
    for stream, first in [(HEAD, FIRST), (b"\x20\x00\x00", 0), (HEAD + plain(1)[:-1], FIRST), (b"", 0)]:
        got, stop, stats = capi.bam_walk(ctx, stream, first, N_REF)
        assert len(got) == 0 and stop == first and stats["chunks"] == 1
        assert all(len(a) == 0 for a in capi.bam_match_segments(ctx, stream, got, N_REF))


# ---- the segments ------------------------------------------------------------------------------------------------------------------
def test_segment_rules(ctx):
    n_ref = 3
    ops40 = cigar_words("1M1D" * 40)
    cg = lambda name, aux, pos=7: record(name, 0, 2, pos, 30, [(40 << 4) | 4, (80 << 4) | 3], l_seq=40, aux=aux)
    recs = [record("m", 0, 0, 100, 60, "20S80M"),
            record("rev", 0x10, 1, 5, 60, "50M")]
    recs += [record(f"f{f:x}", f, 0, 10, 60, "10M") for f in (0x4, 0x100, 0x200, 0x400, 0x800)]         # only 0x800 counts
    recs += [record("tid-1", 0, -1, 10, 60, "10M"), record("tid3", 0, 3, 10, 60, "10M"), record("tid9", 0, 9, 10, 60, "10M"),
             record("pos-1", 0, 1, -1, 60, "10M"),
             record("zero", 0, 1, 20, 60, "0M5M0D0=3X0N"),
             record("mix", 0, 2, 1000, 60, "5S10M2D3I7M100N4=1X2P6M5H"),
             record("nocig", 0, 1, 30, 60, "", l_seq=12),
             cg("cg", aux_i("NM", 1) + aux_B("CG", "I", ops40)),
             cg("cg_i", aux_B("CG", "i", ops40)),                                                         # subtype i is taken too
             cg("cg_wrong_type", aux_B("CG", "S", [w & 0xffff for w in ops40])),                          # ignored: the placeholder stays
             cg("cg_z", aux_Z("CG", "80M")),
             cg("cg_short", aux_B("CG", "I", [(5 << 4) | 0])),                                            # count < n_cigar_op: ignored
             cg("cg_twice", aux_B("CG", "S", [1, 2]) + aux_B("CG", "I", ops40)),                          # the first CG tag decides
             cg("cg_twice2", aux_B("CG", "I", ops40) + aux_B("CG", "I", cigar_words("40M"))),
             cg("cg_behind_unknown", b"XQ?" + b"abcd" + aux_B("CG", "I", ops40)),                        # unknown type: the scan stops
             cg("cg_behind_open_z", b"XZZ" + b"no end" ),                                                # a string that runs past the record
             cg("cg_negpos", aux_B("CG", "I", ops40), pos=-1),
             record("fake", 0, 2, 9, 30, [(50 << 4) | 4, (60 << 4) | 3], l_seq=50),
             record("last", 0, 0, 4000, 60, "30=5X15M", aux=aux_A("XA", "q"))]
    stream = HEAD + b"".join(recs)
    want, _ = check_walk(ctx, stream, FIRST, 256, n_ref)
    assert len(want) == len(recs)
    exp = serial_segments(stream, want, n_ref)
    # the restatement itself, on what can be said by hand
    assert exp[:3] == [(0, 100, 80), (1, 5, 50), (0, 10, 10)]
    assert (1, 20, 5) in exp and (1, 25, 3) in exp and (2, 1000, 10) in exp and (2, 1012, 7) in exp and (2, 1119, 4) in exp and (2, 1124, 6) in exp
    assert sum(1 for s in exp if s[0] == 2 and s[2] == 1 and 7 <= s[1] < 7 + 80) == 40 * 3            # cg, cg_i, cg_twice2: the tag is taken
    seg = capi.bam_match_segments(ctx, stream, want, n_ref)
    assert list(zip(*(a.tolist() for a in seg))) == exp
    # no records: no segments, and the count alone
    assert all(len(a) == 0 for a in capi.bam_match_segments(ctx, stream, [], n_ref))
