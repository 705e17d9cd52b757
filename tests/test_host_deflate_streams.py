"""The hand-written DEFLATE streams of tests/deflate_streams.py on a CPU: zlib's verdict on every one is the catalogue's and the token
model equals zlib's bytes on the valid ones; the loader's own decoder (host/inflate_fast.hpp, both of its builds) is held to the same
catalogue through `inflate_selftest streams`, as built and under ASan + UBSan with every buffer exactly as long as stated; and the files
whose matches reach before the start of their member are refused by zlib and declined by the chain walk of host/gzip_member.hpp."""
import os
import struct
import subprocess
import zlib

import pytest

from tests import deflate_streams as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = ("inflate_selftest", "inflate_selftest_asan")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in TOOLS], check=True, stdout=subprocess.DEVNULL)


def test_zlib_verdict_is_the_catalogues_and_the_model_equals_zlib():
    cat = ds.catalogue()
    names = [c.name for c in cat]
    assert len(set(names)) == len(names)
    assert sum(c.text is not None for c in cat) >= 35 and sum(c.text is None for c in cat) >= 21
    for c in cat:
        ok, got = ds.zlib_says(c.raw, c.out_len)
        assert ok == (c.text is not None), c.name
        if ok:
            assert got == c.text and len(c.text) == c.out_len and c.out_len <= 65536, c.name
            d = zlib.decompressobj(-15)                                # the stream ends where the catalogue says it does
            d.decompress(c.raw)
            assert d.eof and len(d.unused_data) == c.tail, c.name
        elif c.why:                                                    # refused for the reason the case is named after
            with pytest.raises(zlib.error, match=c.why):
                zlib.decompressobj(-15).decompress(c.raw)
        else:                                                          # a sound stream that gives one byte more than stated
            d = zlib.decompressobj(-15)
            assert len(d.decompress(c.raw)) == c.out_len + 1 and d.eof, c.name


def test_long_streams_equal_zlib_and_start_blocks_on_every_bit_phase():
    for g in ds.long_streams():
        assert 300_000 <= len(g.text) <= 1_000_000, g.name
        assert zlib.decompress(g.raw, -15) == g.text, g.name
        dyn = [bit for bit, kind in g.starts if kind == 2]
        gaps = [b - a for a, b in zip(dyn, dyn[1:])]
        assert len(dyn) >= 90 and max(gaps) <= 8 * 4096, g.name         # a stride of 512 or 1024 bytes finds tens of them
    c = ds.long_streams()[2]
    assert {kind for _, kind in c.starts} == {0, 1, 2}
    assert {bit % 8 for bit, kind in c.starts if kind == 2} == set(range(8))


def test_files_that_reach_before_their_member_are_refused_by_zlib():
    files = ds.reach_before_files()
    assert set(files) == {"one_member", "second_of_two_members"}
    for name, (blob, bit, member) in files.items():
        text, msg = ds.zlib_file_says(blob)
        assert text is None and "invalid distance too far back" in msg, name
        # the offending block is the first non-final dynamic block behind more than 16 KiB of compressed data of its member ...
        three = int.from_bytes(blob[bit >> 3:(bit >> 3) + 2], "little") >> (bit & 7)
        assert three & 7 == 4, name
        assert blob[member:member + 4] == b"\x1f\x8b\x08\x00"
        assert bit - 8 * (member + 10) > 8 * (16 << 10), name
        assert ds.REACH_FIRST_BLOCK < ds.REACH_DISTANCE <= ds.WINDOW
    # ... and the first member of the second file is sound on its own
    blob = files["second_of_two_members"][0]
    d = zlib.decompressobj(31)
    assert len(d.decompress(blob)) > ds.WINDOW and d.eof and d.unused_data[:2] == b"\x1f\x8b"


def container(cases):
    return b"".join(struct.pack("<II", len(c.raw), c.out_len) + c.raw for c in cases)


@pytest.mark.parametrize("slack", (0, 8))
@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_inflate_fast_holds_to_the_catalogue(tool, slack, tmp_path):
    cat = ds.catalogue()
    path = tmp_path / "streams.bin"
    path.write_bytes(container(cat))
    p = subprocess.run([os.path.join(BIN, tool), "streams", str(path), str(slack)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-3000:]
    lines = p.stdout.decode().splitlines()
    assert len(lines) == len(cat)
    for i, (c, ln) in enumerate(zip(cat, lines)):
        f = ln.split()
        assert f[0] == str(i) and f[1] == "fast" and f[3] == "plain" and f[5] == "crc", ln
        fast, plain, crc = int(f[2]), int(f[4]), int(f[6], 16)
        if c.text is not None:                                         # valid: accepted by both builds, zlib's bytes
            assert fast == 1 and plain == 1, (c.name, ln)
            assert crc == zlib.crc32(c.text), c.name
        else:
            assert fast == 0 and plain == 0, (c.name, ln)
