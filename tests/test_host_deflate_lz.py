"""The member encoder of palace_bgzf_deflate_lz on a CPU (palace_amd/host/deflate_lz_selftest_main.cpp runs the phases of
csrc/deflate_lz.hpp and csrc/deflate_enc.hpp thread by thread) over the catalogue of tests/deflate_lz_cases.py, at the four
misalignments of the text: every member is, byte for byte, the member of the exact model (tests/deflate_lz_model.py), the reader
written from RFC 1951 (tests/deflate_read.py) gives the model's tokens back, zlib inflates it to the piece, CRC-32 and ISIZE are
right, and no member is longer than n + 31 bytes.  The model alone is held to what the catalogue plants: the window's edge, the chunk
borders, the round rule, the bucket shared by two strings -- and to the condition of the coder's being: on text shaped like a BAM it
finds matches and writes fewer bytes than the previous-line coder.  The sanitizer build of the same program runs the catalogue too.
The device is held to the same members in tests/test_gpu_bgzf_deflate_lz.py."""
import os
import struct
import subprocess
import zlib

import pytest

from tests import deflate_enc_checks as ck
from tests import deflate_lz_cases as lc
from tests import deflate_lz_model as lz
from tests import deflate_read as dr

TOOL = os.path.join(ck.ROOT, "palace_amd", "bin", "deflate_lz_selftest")
TOOL_ASAN = TOOL + "_asan"


def named():
    return lc.cases()


@pytest.fixture(scope="module")
def members(tmp_path_factory):
    ck.make(TOOL)
    tmp = tmp_path_factory.mktemp("lz")
    pieces = [p for _, p in named()]
    return [ck.host_members(tmp, pieces, mis, tool=TOOL) for mis in range(4)]


# ---- the model alone ----------------------------------------------------------------------------------------------------------------

def test_the_models_tokens_spell_the_piece_and_stay_inside_their_chunks():
    for name, piece in named():
        tokens = lz.tokens_of(piece)
        assert lz.dm.text_of(tokens) == piece, name
        chunk, p = lz.chunk_of(len(piece)) if piece else 1, 0
        for t in tokens:
            k = 1 if t[0] == "lit" else t[1]
            assert p // chunk == (p + k - 1) // chunk, (name, p, t)
            assert t[0] == "lit" or (3 <= t[1] <= 258 and 1 <= t[2] <= 32768 and t[2] <= p), (name, p, t)
            p += k


def test_the_window_ends_at_32768():
    by = dict(named())
    at, k = lc.PLANTED["distance_32768"]
    got = lc.tokens_at(by["distance_32768"], at, k)
    assert all(t[0] == "match" and t[2] == 32768 for _, t in got) and sum(t[1] for _, t in got) == k, got[:5]
    assert len(got) == len({p // lz.chunk_of(len(by["distance_32768"])) for p in range(at, at + k)})       # one token per chunk it touches
    at, k = lc.PLANTED["distance_32769"]
    assert all(t[0] == "lit" for _, t in lc.tokens_at(by["distance_32769"], at, k))


@pytest.mark.parametrize("k", [258, 259, 600])
def test_a_long_repeat_is_one_match_per_chunk(k):
    piece = dict(named())[f"repeat_{k}"]
    at, _ = lc.PLANTED[f"repeat_{k}"]
    chunk = lz.chunk_of(len(piece))
    assert chunk == 40 and at % chunk == 0
    got = lc.tokens_at(piece, at, k)
    assert got == [(at + c, ("match", min(chunk, k - c), 8000)) for c in range(0, k, chunk)]     # (258 = 6 * 40 + 18, 259 = 6 * 40 + 19, 600 = 15 * 40)


def test_a_repeat_across_a_chunk_border_is_two_tokens():
    by = dict(named())
    at, k = lc.PLANTED["repeat_inside_a_chunk"]
    assert lc.tokens_at(by["repeat_inside_a_chunk"], at, k) == [(at, ("match", 30, 8005))]
    at, k = lc.PLANTED["repeat_across_a_chunk_border"]
    assert lc.tokens_at(by["repeat_across_a_chunk_border"], at, k) == [(at, ("match", 15, 8025)), (at + 15, ("match", 15, 8025))]


def test_a_source_in_the_copys_own_round_is_not_found():
    by = dict(named())
    at, k = lc.PLANTED["source_in_the_same_round"]
    assert all(t[0] == "lit" for _, t in lc.tokens_at(by["source_in_the_same_round"], at, k))
    got = lc.tokens_at(by["source_in_the_round_before"], at, k)
    assert got and all(t[0] == "match" and t[2] == 300 for _, t in got)


def test_two_strings_of_one_bucket_compare_unequal():
    a, b = lc.colliding_words()
    assert a != b and lz.hash4(a) == lz.hash4(b)
    piece = dict(named())["equal_hash_different_bytes"]
    at, k = lc.PLANTED["equal_hash_different_bytes"]
    assert piece[at:at + 4] == b and lz.distances(piece)[at] == at - 100           # the candidate is read ...
    assert lc.tokens_at(piece, at, 1) == [(at, ("lit", b[0]))]                     # ... and a literal results


def test_overlapping_copies_are_in_the_catalogue():
    by = dict(named())
    for name in ("one_byte_run", "period_2", "period_3"):
        tokens = lz.tokens_of(by[name])
        assert any(t[0] == "match" and t[2] < t[1] for t in tokens), name
    assert ("match", 128, 1) in lz.tokens_of(by["one_byte_run"])


def test_on_text_shaped_like_a_bam_the_matcher_beats_the_previous_line_coder(tmp_path):
    """the condition of the coder's being, on the model and on the CPU builds of both coders"""
    piece = dict(named())["bam_shaped"]
    assert len(piece) > 60000
    member = lz.member_of(piece)
    assert lz.has_match(member)
    ck.make(ck.TOOL)
    line = ck.host_members(tmp_path, [piece], 0)[0]
    assert zlib.decompress(line, 31) == piece
    print(f"bam_shaped: {len(piece)} bytes; hashed matcher {len(member)}, previous-line coder {len(line)}, zlib level 1 {len(zlib.compress(piece, 1))}")
    assert len(member) < len(line)


# ---- the CPU build against the model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mis", range(4))
def test_every_member_is_the_models_member(members, mis):
    differ = [(name, len(m), len(lz.member_of(piece))) for (name, piece), m in zip(named(), members[mis]) if m != lz.member_of(piece)]
    assert not differ, differ[:10]


def test_the_reader_gives_the_models_tokens_back(members):
    kinds = {}
    for (name, piece), m in zip(named(), members[0]):
        if not piece:
            continue
        s = dr.read(m[18:len(m) - 8], max_out=len(piece))
        b = s.blocks[0]
        assert len(s.blocks) == 1 and b.final == 1 and b.btype in (0, 2), name
        assert b.tokens == (lz.tokens_of(piece) if b.btype == 2 else [("lit", v) for v in piece]), name
        kinds[name] = b.btype
    assert kinds["noise"] == 0 and kinds["size_1"] == 0
    coded = [n for n in kinds if kinds[n] == 2]
    assert set(coded) >= set(lc.PLANTED) | {"one_byte_run", "period_2", "period_3", "bam_shaped", f"size_{lc.MAX_TEXT}", f"size_{lc.R + 1}"}, kinds


def test_zlib_inflates_every_member_to_its_piece_and_the_trailer_is_right(members):
    for mis in range(4):
        for (name, piece), m in zip(named(), members[mis]):
            assert zlib.decompress(m, 31) == piece, (name, mis)
            assert struct.unpack_from("<II", m, len(m) - 8) == (zlib.crc32(piece), len(piece)), (name, mis)
            assert struct.unpack_from("<H", m, 16)[0] == len(m) - 1 and 28 <= len(m) <= len(piece) + 31, (name, mis, len(m))
    by = {name: m for (name, _), m in zip(named(), members[0])}
    assert len(by["noise"]) == 5000 + 31 and len(by["empty"]) == 28


def test_the_sanitizer_build_runs_the_catalogue_clean(members, tmp_path):
    ck.make(TOOL_ASAN)
    pieces = [p for _, p in named()]
    for mis in (0, 3):
        assert ck.host_members(tmp_path, pieces, mis, tool=TOOL_ASAN) == members[mis]


def test_a_file_through_the_tool_inflates_in_zlib(tmp_path):
    ck.make(TOOL)
    text = lc.bam_shaped(seed=5, records=700)[:lc.MAX_TEXT] + lc.bam_shaped(seed=6, records=300)
    src, out = str(tmp_path / "text"), str(tmp_path / "out.gz")
    open(src, "wb").write(text)
    ck.run_tool(TOOL, [src, out])
    blob, got = open(out, "rb").read(), b""
    while blob:
        d = zlib.decompressobj(31)
        got += d.decompress(blob)
        assert d.eof
        blob = d.unused_data
    assert got == text


def test_the_tools_usage():
    ck.make(TOOL)
    p = subprocess.run([TOOL, "batch", os.devnull, os.devnull], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and b"Usage" in p.stderr


@pytest.mark.parametrize("which", ["bam_case", "sam_case"])
def test_the_cli_fixtures_meet_the_condition_on_the_model(tmp_path, which):
    """the streams `bamsort --lz` and `samview --lz` are tested on (tests/test_gpu_bamsort_lz_cli.py): by the model alone the members hold
    matches and are fewer bytes in all than the previous-line coder's (its CPU build) for the same text"""
    from tests import bamsort_lz_cases as cl
    pieces = cl.pieces(getattr(cl, which)()[1])
    assert len(pieces) >= 5
    mine = [lz.member_of(p) for p in pieces]
    assert all(lz.has_match(m) for m in mine)
    ck.make(ck.TOOL)
    line = ck.host_members(tmp_path, pieces, 0)
    print(f"{which}: {sum(map(len, pieces))} bytes; hashed matcher {sum(map(len, mine))}, previous-line coder {sum(map(len, line))}")
    assert sum(map(len, mine)) < sum(map(len, line))
