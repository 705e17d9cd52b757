"""palace_bgzf_deflate + palace_bgzf_compact (csrc/bgzf_deflate.hip: one workgroup per BGZF member) through capi: every member
inflates to its piece in zlib (which checks CRC-32 and ISIZE) and in palace_bgzf_inflate, BSIZE is the member's length, the bytes
do not depend on the run or on the members' order, and depth-like text comes out no more than 1.25 x as large as zlib level 6
makes it (a literal-only or fixed-Huffman coder is at 2 x)."""
import struct
import zlib

import numpy as np
import pytest

from palace_amd import capi
from tests import deflate_pieces as dp

pytestmark = pytest.mark.gpu


def split(data, moff):
    return [data[int(a):int(b)] for a, b in zip(moff[:-1], moff[1:])]


def device_inflate(ctx, members, sizes):
    """the members' DEFLATE streams through palace_bgzf_inflate -> (status, [bytes])"""
    blob, in_off, out_off, o = bytearray(), [], [], 0
    for m, k in zip(members, sizes):
        in_off.append(len(blob) + 18)
        blob += m
        out_off.append(o)
        o += k
    blob += bytes(8)
    n = len(members)
    bufs = [ctx.upload(np.frombuffer(bytes(blob), np.uint8)), ctx.upload(np.array(in_off, np.int64)),
            ctx.upload(np.array([len(m) - 26 for m in members], np.int32)), ctx.upload(np.array(out_off, np.int64)),
            ctx.upload(np.array(sizes, np.int32)), ctx.upload(np.zeros(o + 8, np.uint8)), ctx.upload(np.full(n, -1, np.int32))]
    capi._check(capi.lib().palace_bgzf_inflate(ctx.h, bufs[0].ptr, n, *(b.ptr for b in bufs[1:])), "palace_bgzf_inflate")
    ctx.sync()
    st, out = bufs[6].to_host(), bufs[5].to_host().tobytes()
    for b in bufs:
        b.free()
    return st, [out[a:a + k] for a, k in zip(out_off, sizes)]


@pytest.fixture(scope="module")
def batch():
    named = dp.pieces()
    pieces = [p for _, p in named]
    with capi.Ctx(0) as ctx:
        data, moff = capi.bgzf_deflate(ctx, pieces, lead=1)
        again, moff2 = capi.bgzf_deflate(ctx, pieces, lead=1)
        rev, moff_r = capi.bgzf_deflate(ctx, pieces[::-1], lead=2)
        members = split(data, moff)
        st, inflated = device_inflate(ctx, members, [len(p) for p in pieces])
    return dict(named=named, members=members, again=split(again, moff2), rev=split(rev, moff_r)[::-1], st=st, inflated=inflated)


def test_every_member_is_a_bgzf_member_of_its_piece(batch):
    for (name, piece), m in zip(batch["named"], batch["members"]):
        assert m[:4] == b"\x1f\x8b\x08\x04" and m[10:16] == b"\x06\x00BC\x02\x00", name
        assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1 <= 65535, name
        assert zlib.decompress(m, wbits=31) == piece, name
        assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(piece), len(piece)), name
    by = dict(zip((n for n, _ in batch["named"]), batch["members"]))
    assert by["empty"] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert len(by["random"]) == 18 + 5 + dp.MAX_TEXT + 8 <= 65311 and by["random"][18] == 1        # a stored block
    for name in ("newlines", "one_value", "no_newline", "rolls", "mid_line", "fibonacci"):
        assert by[name][18] & 7 == 5, name                                  # BFINAL, BTYPE = 10
        assert len(by[name]) < len(dict(batch["named"])[name]), name


def test_the_device_inflater_reads_every_member(batch):
    assert (batch["st"] == 0).all(), batch["st"]
    for (name, piece), got in zip(batch["named"], batch["inflated"]):
        assert got == piece, name


def test_same_bytes_on_every_run_and_in_every_order(batch):
    for (name, _), a, b, r in zip(batch["named"], batch["members"], batch["again"], batch["rev"]):
        assert a == b, name
        assert a == r, name


def test_depth_text_is_close_to_zlib_level_6():
    pieces = dp.cut(dp.depth_text())
    with capi.Ctx(0) as ctx:
        data, moff = capi.bgzf_deflate(ctx, pieces)
    members = split(data, moff)
    assert all(zlib.decompress(m, wbits=31) == p for m, p in zip(members, pieces))
    ours, theirs = len(data), sum(len(zlib.compress(p, 6)) for p in pieces)
    print(f"depth text: {sum(map(len, pieces))} bytes in {len(pieces)} members -> {ours} (device), {theirs} (zlib level 6): ratio {ours / theirs:.4f}")
    assert ours <= 1.25 * theirs
