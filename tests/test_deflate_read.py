"""tests/deflate_read.py (the DEFLATE reader the BGZF writer's tests read members with) against two independent statements of what
a stream means: zlib, whose streams at every strategy it must turn into tokens that give the text back, and the hand-written
catalogue of tests/deflate_streams.py, whose valid cases it must read to their text and whose malformed ones it must refuse."""
import zlib

import numpy as np
import pytest

from tests import deflate_pieces as dp
from tests import deflate_read as dr
from tests import deflate_streams as ds


def texts():
    rng = np.random.default_rng(1951)
    lines = dp.depth_lines(b"NODE_1_length_5000_cov_9.75", range(1, 3001), rng.integers(5, 120, 3000).tolist())
    return [("empty", b""), ("one_byte", b"q"), ("depth_lines", lines), ("run", b"z" * 70000),
            ("noise", rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()),
            ("words", b" ".join(rng.choice([b"alpha", b"beta", b"gamma", b"delta\n", b"epsilon"], 9000).tolist()))]


def raw_deflate(text, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(text) + c.flush()


@pytest.mark.parametrize("how", ["level0", "level1", "level6", "level9", "fixed"])
def test_zlib_output_reads_to_tokens_that_give_the_text(how):
    for name, text in texts():
        raw = raw_deflate(text, 6, zlib.Z_FIXED) if how == "fixed" else raw_deflate(text, int(how[-1]))
        s = dr.read(raw + b"\xa5\x5a")
        assert ds.model(dr.stream_tokens(s.tokens)) == text, name
        assert (s.bits + 7) // 8 == len(raw) and s.blocks[-1].final == 1 and not any(b.final for b in s.blocks[:-1]), name
        kinds = {b.btype for b in s.blocks}
        assert kinds <= ({0} if how == "level0" else {0, 1} if how == "fixed" else {0, 1, 2}), name     # (zlib stores noise at any strategy)
        assert how != "fixed" or name == "noise" or kinds == {1}, name
        for b in s.blocks:
            assert len(b.tokens) == len(b.symbols) or b.btype == 0
            if b.btype == 2:
                assert len(b.lit_lens) == b.hlit and len(b.dist_lens) == b.hdist and 4 <= b.hclen <= 19, name
                sent = sum((1, 3 + x, 3 + x, 11 + x)[max(0, sym - 15)] for sym, x in b.cl_syms)
                assert sent == b.hlit + b.hdist, name


def test_every_valid_hand_written_stream_reads_to_its_text():
    for c in ds.valid_cases():
        s = dr.read(c.raw)
        assert ds.model(dr.stream_tokens(s.tokens)) == c.text, c.name
        assert (s.bits + 7) // 8 == len(c.raw) - c.tail, c.name


def test_malformed_streams_are_refused():
    for c in ds.invalid_cases():                                          # (a sound stream of one byte too many: refused by max_out)
        with pytest.raises(dr.DeflateError):
            dr.read(c.raw, max_out=c.out_len)
            pytest.fail(c.name)
    for raw, why in ((bytes([0b111]), "BTYPE 11"), (bytes([1, 5, 0, 0xfa, 0xfe]), "NLEN"), (bytes([1, 5, 0, 0xfa, 0xff, 1]), "ends"),
                     (bytes([0b011]), "ends")):
        with pytest.raises(dr.DeflateError, match=why):
            dr.read(raw)
