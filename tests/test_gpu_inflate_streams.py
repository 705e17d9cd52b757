"""The device's two DEFLATE decoders on streams written by hand (tests/deflate_streams.py) -- the regions of RFC 1951 zlib's encoder never
visits, which every valid stream of test_gpu_inflate.py and test_gpu_gzip_inflate.py comes from: no distance code, a lone 1-bit distance
code, distance 32 768, length 258 as 284 + 31, 15-bit codes with all extra bits set, a lone end-of-block code, stored blocks from every
bit phase, overlapping copies around a wavefront's width.  The reference is the token model of that module, which the CPU test
(test_host_deflate_streams.py) holds equal to zlib.

palace_bgzf_inflate: a valid stream is decoded to the model's bytes with status 0 -- never merely "refused or equal" --, an invalid one is
refused.  palace_gzip_inflate: every valid stream stays on the device path (fallback 0) and gives the model's text, every invalid one is
declined with no text, and a file whose match reaches before the start of its member is declined as PALACE_GZ_MARKER in whichever chunk
the match lies, where zlib says "invalid distance too far back"."""
import pytest

from palace_amd import capi, synth
from tests import deflate_streams as ds
from tests import gz_util as gz
from tests.test_gpu_gzip_inflate import check
from tests.test_gpu_inflate import run_members

pytestmark = pytest.mark.gpu

PALACE_GZ_MARKER = 11


def test_bgzf_inflate_holds_to_the_catalogue():
    cat = ds.catalogue()
    rng = synth.rng_for(1951)
    copies = 4                                                          # every stream at four alignments of its input and output
    members = [(c.raw, c.out_len) for c in cat] * copies
    with capi.Ctx(0) as ctx:
        st, got = run_members(ctx, members, rng)
    wrong = []
    for i, (s, g) in enumerate(zip(st.tolist(), got)):
        c = cat[i % len(cat)]
        if c.text is not None:
            if s != 0:
                wrong.append((c.name, "a valid stream was refused", s))
            elif g != c.text:
                at = next(k for k in range(len(g)) if g[k] != c.text[k])
                wrong.append((c.name, "bytes differ from the model's", at))
        elif s == 0:
            wrong.append((c.name, "a stream zlib refuses was accepted", 0))
    assert not wrong, wrong
    assert sum(c.text is not None for c in cat) >= 35 and sum(c.text is None for c in cat) >= 21


def test_gzip_inflate_small_valid_streams():
    # (the stream with bytes behind it is left to the BGZF decoder: behind a gzip member's DEFLATE data lies its trailer, so wrapped
    # without those bytes it is its sibling, and with them it is a file with a wrong trailer)
    cat = [c for c in ds.catalogue() if c.text is not None and not c.tail]
    assert len(cat) >= 34
    with capi.Ctx(0) as ctx:
        for c in cat:
            print(c.name)
            st = check(ctx, gz.gzip_wrap(c.raw, c.text), c.text)
            assert st["members"] == 1 and st["chunks_accepted"] >= 1
        by_name = {c.name: c for c in cat}
        four = [by_name[n] for n in ("lone_distance_code_symbol_29", "fifteen_bit_codes_all_extra_bits_set", "hlit_286_hdist_30_every_symbol_used",
                                     "distances_1_to_69_by_lengths_3_to_258")]
        blob = b"".join(gz.gzip_wrap(c.raw, c.text, fname=c.name.encode()) for c in four)
        want = b"".join(c.text for c in four)
        assert check(ctx, blob, want)["members"] == 4
        assert check(ctx, blob, want, stride=512)["members"] == 4


@pytest.mark.parametrize("which", (0, 1, 2), ids=("far_matches", "alternating_code_sets", "every_block_type"))
def test_gzip_inflate_long_streams(which):
    g = ds.long_streams()[which]
    blob = gz.gzip_wrap(g.raw, g.text)
    with capi.Ctx(0) as ctx:
        st = check(ctx, blob, g.text)
        assert st["chunks_accepted"] >= 8, st
        for stride in (512, 1024):
            st = check(ctx, blob, g.text, stride=stride, span=len(blob) // 4 + 1)
            assert st["chunks_accepted"] >= 30 and st["spans"] >= 4, st


def test_gzip_inflate_declines_every_invalid_stream():
    cat = [c for c in ds.catalogue() if c.text is None]
    assert len(cat) >= 21
    with capi.Ctx(0) as ctx:
        for c in cat:
            blob = gz.gzip_wrap(c.raw, bytes(c.out_len))
            assert ds.zlib_file_says(blob)[0] is None, c.name
            text, st = capi.gzip_inflate(ctx, blob, check_guards=True)
            print(c.name, "fallback", st["fallback"])
            assert st["guards_bad"] == 0, c.name
            assert st["fallback"] != 0 and text is None, (c.name, st)


@pytest.mark.parametrize("name", ("one_member", "second_of_two_members"))
def test_gzip_inflate_declines_a_match_that_reaches_before_its_member(name):
    """The match lies in a chunk of its own behind the chunk that opens the member, at a stride of 512 bytes and at the default one; the
    member's trailer carries the CRC-32 and ISIZE of the text a decoder gives that resolves the match from the window it carries (zeros,
    or the previous member's text), so neither stands against the file."""
    blob, _, _ = ds.reach_before_files()[name]
    text, msg = ds.zlib_file_says(blob)
    assert text is None and "invalid distance too far back" in msg
    with capi.Ctx(0) as ctx:
        for kw in ({"stride": 512}, {}):
            text, st = capi.gzip_inflate(ctx, blob, check_guards=True, **kw)
            print(name, kw, {k: v for k, v in st.items() if not k.startswith("ms_")})
            assert st["guards_bad"] == 0
            assert st["fallback"] == PALACE_GZ_MARKER and text is None, st
            assert st["chunks_found"] >= 1
