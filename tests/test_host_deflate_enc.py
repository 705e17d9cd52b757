"""The member encoder of palace_bgzf_deflate run on a CPU (palace_amd/host/deflate_selftest_main.cpp runs the phases of
csrc/deflate_enc.hpp thread by thread): every piece of tests/deflate_pieces.py leaves as a BGZF member that zlib inflates to the
piece -- CRC-32 and ISIZE checked by zlib, BSIZE by the reader written from the specification -- and depth-like text comes out
no more than 1.25 x as large as zlib level 6 makes it.  The same checks run against the device in tests/test_gpu_bgzf_deflate.py."""
import os
import subprocess
import zlib

import pytest

from tests import deflate_pieces as dp
from tests import tabix_reader as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "palace_amd", "bin", "deflate_selftest")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host"), os.path.join("..", "bin", "deflate_selftest")], check=True,
                   stdout=subprocess.DEVNULL)


def encode(tmp_path, text):
    src, gz = str(tmp_path / "in.txt"), str(tmp_path / "out.gz")
    open(src, "wb").write(text)
    p = subprocess.run([TOOL, src, gz], stdout=subprocess.PIPE, check=True)
    return open(gz, "rb").read(), p.stdout.decode()


@pytest.mark.parametrize("name,piece", dp.pieces(), ids=[n for n, _ in dp.pieces()])
def test_piece_inflates_to_itself(tmp_path, name, piece):
    data, said = encode(tmp_path, piece)
    assert data[-28:] == tr.EOF_MEMBER
    members = tr.bgzf_members(data)                                       # BSIZE, CRC-32, ISIZE of every member
    assert b"".join(t for _, t in members) == piece
    assert len(members) == (2 if piece else 1)
    if piece:
        first = data[:members[1][0]]
        assert zlib.decompress(first, wbits=31) == piece and len(first) <= 65536
    if name == "random":
        assert len(first) == 18 + 5 + len(piece) + 8 and "1 stored" in said
    elif len(piece) > 1000:                                              # (a byte or two are shorter stored than behind a block header)
        assert "0 stored" in said


def test_depth_text_is_close_to_zlib_level_6(tmp_path):
    text = dp.depth_text()
    data, _ = encode(tmp_path, text)
    members = tr.bgzf_members(data)
    assert b"".join(t for _, t in members) == text and [len(t) for _, t in members[:-2]] == [dp.MAX_TEXT] * (len(members) - 2)
    ours = len(data) - 28
    theirs = sum(len(zlib.compress(p, 6)) for p in dp.cut(text))
    print(f"depth text: {len(text)} bytes -> {ours} (this encoder), {theirs} (zlib level 6): ratio {ours / theirs:.4f}")
    assert ours <= 1.25 * theirs
