"""palace_sam_lines, palace_sam_plan and palace_sam_encode (palace_amd/csrc/sam.hip) through the C ABI on texts built from the cases
of tests/sam_cases.py.  Expectations come from that Python restatement of DESIGN.md section 8, never from the device: the line
starts, the per-line sizes, the offsets, the record starts and every byte of the stream, with the bytes in front of the first record
and behind the last untouched."""
import numpy as np
import pytest

from palace_amd import capi
from tests import sam_cases as sc

pytestmark = pytest.mark.gpu

T = capi.SAM_TILE
HEAD = bytes(range(101))                    # a stand-in for the BAM header; its odd length puts the records at no alignment


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx() as c:
        yield c


def run(ctx, text, mask=0, head=HEAD):
    """the three calls on one text, each checked against the restatement; -> the first fault (line, code) or None"""
    starts, n_header, n_align, err_line, err_code = capi.sam_lines(ctx, text)
    lines = sc.split_lines(text)
    want_starts = np.cumsum([0] + [len(l) + 1 for l in lines])
    assert starts.tolist() == want_starts.tolist()                           # (a last line without LF ends one byte past the text)
    assert (n_header, n_align, err_line, err_code) == sc.lines_verdict(text)
    if err_code:
        return err_line, err_code
    names = [n for n, _ in sc.header_of(text)[2]]
    recs, sizes, first = sc.text_verdict(text, mask)
    res = capi.sam_encode(ctx, text, starts, n_header, names, mask, head)
    if first:
        assert (res["err_line"], res["err_code"]) == first
        return first
    assert (res["err_line"], res["err_code"]) == (0, 0)
    off = np.cumsum([len(head)] + sizes)
    kept = [k for k, s in enumerate(sizes) if s]
    assert res["size"].tolist() == sizes and res["off"].tolist() == off.tolist()
    assert res["ord"].tolist() == np.cumsum([0] + [1 if s else 0 for s in sizes])[:-1].tolist()
    assert (res["kept"], res["dropped"], res["bytes"]) == (len(kept), len(sizes) - len(kept), int(off[-1]))
    assert res["starts"].tolist() == [int(off[k]) + 4 for k in kept]
    assert res["stream"] == head + b"".join(recs) + b"\xaa" * 16            # every byte, and nothing outside [off[0], off[n])
    assert capi.sam_plan(ctx, text, starts, n_header, names, mask, len(head))["off"].tolist() == off.tolist()
    return None


def padded(line, length):
    """`line` with a Z tag that makes it `length` bytes long"""
    pad = length - len(line) - 6
    assert pad >= 0
    return line + b"\tXP:Z:" + b"p" * pad


GOOD = sc.SPEC_READS[0]


def test_hand_cases_in_one_text(ctx):
    lines = sc.HAND_VALID
    for mask in (0, 0x800, 4):
        assert run(ctx, sc.HEADER + b"\n".join(lines) + b"\n", mask) is None
        assert run(ctx, sc.HEADER + b"\n".join(lines), mask) is None          # the last line without LF
    assert run(ctx, b"\n".join(l for l in lines if b"\t*\t" in l[:12]) + b"\n") is None   # no header at all: no target, RNAME '*' only


def test_smallest_texts(ctx):
    for text in (b"", sc.HEADER, sc.HEADER[:-1], b"@CO", sc.HEADER + GOOD, sc.HEADER + GOOD + b"\n", sc.SPEC_READS[1].replace(b"ref", b"*")):
        assert run(ctx, text) is None, text
    assert run(ctx, b"\n") == (1, sc.EEMPTY) and run(ctx, sc.HEADER + b"\n") == (6, sc.EEMPTY)
    assert run(ctx, sc.HEADER + GOOD + b"\n\n") == (7, sc.EEMPTY) and run(ctx, GOOD.replace(b"=", b"*") + b"\n@CO\n") == (2, sc.EAT)
    assert run(ctx, sc.HEADER + GOOD + b"\n@CO\tx\n\n" + GOOD + b"\n\n") == (7, sc.EAT)   # the smallest line number, whatever the fault


@pytest.mark.parametrize("begin", [T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_lines_that_begin_around_a_tile_border(ctx, begin):
    first = padded(sc.SPEC_READS[1], begin - len(sc.HEADER) - 1)
    text = sc.HEADER + first + b"\n" + b"\n".join(sc.SPEC_READS[2:]) + b"\n"
    assert text[begin - 1:begin] == b"\n"
    assert run(ctx, text, 0x800) is None
    assert run(ctx, text[:begin]) is None and run(ctx, text[:begin - 1]) is None     # the text ends with and without the LF at the border
    assert run(ctx, text[:begin + 1]) == (7, sc.EFIELDS)                              # one byte of a line behind it


def test_line_lengths_and_seq_lengths(ctx):
    rng = np.random.default_rng(3)
    short = b"q\t0\t*\t0\t0\t*\t*\t0\t0\tAC\t*"
    lines = [padded(short, n) for n in (63, 64, 65, 127, 128, 129, 191, 192, 193)]
    lines += [sc.valid_line(rng, seq_len=n) for n in (0, 1, 2, 63, 64, 65, 127, 128, 129) for _ in range(3)]
    lines += [padded(short, 3 * T + 5),                                      # a line longer than a tile, and longer than two
              b"long\t0\tref\t5\t9\t5000M\t*\t0\t0\t" + b"ACGTN" * 1000 + b"\t" + bytes(33 + k % 94 for k in range(5000)),
              b"ops\t0\tref\t5\t9\t" + b"1M2D" * 150 + b"\t*\t0\t0\t" + b"A" * 150 + b"\t*",      # more ops than a wave has lanes
              b"n" * 254 + b"\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*",
              short + b"".join(b"\tX%c:i:%d" % (65 + k % 26, k * 37 - 2000) for k in range(64)),            # exactly one batch of tags
              short + b"".join(b"\tX%c:Z:%s" % (65 + k % 26, b"z" * (k % 7)) for k in range(65)),
              short + b"".join(b"\tY%c:%s" % (65 + k % 26, [b"A:x", b"i:-70000", b"Z:" + b"s" * 70, b"H:0aF1", b"B:s,-1,2", b"B:I"][k % 6]) for k in range(200))]
    assert run(ctx, sc.HEADER + b"\n".join(lines) + b"\n") is None
    assert run(ctx, sc.HEADER + b"\n".join(reversed(lines))) is None


def test_dropped_lines(ctx):
    rng = np.random.default_rng(5)
    lines = [sc.valid_line(rng).split(b"\t") for _ in range(300)]
    supp = [b"\t".join(f[:1] + [b"2048"] + f[2:]) for f in lines]
    prim = [b"\t".join(f[:1] + [b"16"] + f[2:]) for f in lines]
    assert run(ctx, sc.HEADER + b"\n".join(supp) + b"\n", 0x800) is None      # all lines dropped
    assert run(ctx, sc.HEADER + b"\n".join(s if k & 1 else p for k, (s, p) in enumerate(zip(supp, prim))) + b"\n", 0x800) is None
    assert run(ctx, sc.HEADER + b"\n".join(p if k & 1 else s for k, (s, p) in enumerate(zip(supp, prim))) + b"\n", 0x810) is None


def test_more_targets_than_16_bits(ctx):
    header = b"".join(b"@SQ\tSN:t%d\tLN:%d\n" % (k, 1000 + k) for k in range(70000))
    lines = [b"r%d\t0\tt%d\t7\t1\t2M\t%s\t9\t0\tAC\t*" % (k, k, m) for k, m in ((0, b"t69999"), (65535, b"="), (65536, b"t65535"), (69999, b"*"))]
    text = header + b"\n".join(lines) + b"\n"
    assert run(ctx, text) is None
    rec = sc.text_verdict(text)[0][2]
    assert int.from_bytes(rec[4:8], "little") == 65536 and int.from_bytes(rec[24:28], "little") == 65535
    assert run(ctx, header + lines[0].replace(b"t69999", b"t70000") + b"\n") == (70001, sc.ERNEXT)


def test_the_first_error_is_the_smallest_line(ctx):
    rng = np.random.default_rng(9)
    lines = [sc.valid_line(rng) for _ in range(400)]
    text = lambda ls: sc.HEADER + b"\n".join(ls) + b"\n"
    assert len(text(lines)) > 3 * T
    bad = {k: b"\t".join(fn(lines[k].split(b"\t"), rng)) for k, (fn, _) in zip((399, 57, 200, 58), [sc.DAMAGE[4], sc.DAMAGE[7], sc.DAMAGE[16], sc.DAMAGE[0]])}
    broken = [bad.get(k, l) for k, l in enumerate(lines)]
    assert run(ctx, text(broken)) == (5 + 58, sc.ECIGAR)
    assert run(ctx, text(lines[:399] + [bad[399]])) == (5 + 400, sc.ERNAME)   # the only one, in the last tile
    assert run(ctx, sc.HEADER + b"\n".join(lines[:399] + [bad[399]])) == (5 + 400, sc.ERNAME)
    # an error on a line the mask would have dropped
    supp = lines[10].split(b"\t")
    supp[1], supp[2] = b"2048", b"nowhere"
    assert run(ctx, text(lines[:10] + [b"\t".join(supp)] + lines[11:]), 0x800) == (5 + 11, sc.ERNAME)


def test_every_fault_alone(ctx):
    rng = np.random.default_rng(11)
    for bad, code in sc.HAND_ERRORS + [(b"\t".join(fn(sc.valid_line(rng).split(b"\t"), rng)), code) for fn, code in sc.DAMAGE]:
        assert run(ctx, sc.HEADER + GOOD + b"\n" + bad + b"\n" + GOOD + b"\n", 0xffff) == (7, code), bad


def test_generated_valid_lines(ctx):
    rng = np.random.default_rng(13)
    lines = [sc.valid_line(rng) for _ in range(3000)]
    assert run(ctx, sc.HEADER + b"\n".join(lines) + b"\n", 0x800) is None
