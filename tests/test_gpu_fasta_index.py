"""palace_fasta_index (csrc/path_fasta.hip) at the ABI: FASTA text -> the records a `.fai` holds, or the first fault and its
line, field by field against the Python restatement of tests/path_fasta_cases.py."""
import numpy as np
import pytest

from palace_amd import capi, synth
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu

HAND = pc.hand_fastas(synth.rng_for(3))
MALFORMED = pc.malformed_fastas(synth.rng_for(4))
FIELDS = ("name_off", "name_len", "seq_off", "length", "line_bases", "line_width")


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def check(ctx, text):
    recs, code, line = pc.fasta_index(text)
    st, got, d_text, d_recs = capi.fasta_index(ctx, text)
    d_text.free()
    d_recs.free()
    assert int(st.n_records) == len(recs)
    assert (int(st.error), int(st.bad_line)) == (code, line)
    if code == pc.OK:
        for f in FIELDS:
            want = np.array([r[f] for r in recs], np.int64)
            bad = np.flatnonzero(got[f] != want)
            assert bad.size == 0, (f, int(bad[0]), int(got[f][bad[0]]), int(want[bad[0]]))
    return recs


def test_the_tile_is_the_kernels():
    assert pc.TILE == capi.FASTA_TILE_BYTES


@pytest.mark.parametrize("case", sorted(HAND))
def test_hand_cases(ctx, case):
    recs = check(ctx, HAND[case])
    if case == "three_tiles":
        assert recs[0]["length"] > 3 * pc.TILE
    if case == "many_in_one_tile":
        assert len(recs) == 300 and len(HAND[case]) < pc.TILE
    if case.startswith("lf_on_tile"):
        at = HAND[case].index(b"\n", 4)
        assert at % pc.TILE == (pc.TILE - 1 if case.endswith("last_byte") else 0)


def test_random_records(ctx):
    text = pc.random_fasta(synth.rng_for(8), 2000)
    assert 2 << 20 < len(text) < 5 << 20
    recs = check(ctx, text)
    assert len(recs) == 2000 and min(r["length"] for r in recs) == 0 and max(r["length"] for r in recs) > 2900


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed(ctx, case):
    text, code, line = MALFORMED[case]
    assert pc.fasta_index(text)[1:] == (code, line)
    check(ctx, text)


def test_a_fault_wherever_it_falls(ctx):
    """one fault put into a random line of a random text: the verdict is the restatement's whatever tile, wave or lane it meets"""
    rng = synth.rng_for(9)
    base = pc.random_fasta(rng, 60, max_len=1500)
    assert pc.fasta_index(base)[1] == pc.OK
    lines = base.split(b"\n")
    seen = set()
    for k in range(24):
        ls = list(lines)
        i = int(rng.integers(0, len(ls) - 1))
        kind = k % 4
        if kind == 0:
            ls[i] = ls[i][:len(ls[i]) // 2]                        # a line cut short (a header: another name, or none)
        elif kind == 1:
            ls.insert(i, b"")
        elif kind == 2 and ls[i]:
            ls[i] = ls[i][:-1] + b" "
        else:
            ls[i] = ls[i] + b"AC"
        text = b"\n".join(ls)
        seen.add(pc.fasta_index(text)[1])
        check(ctx, text)
    assert {pc.ERAGGED, pc.EBLANK, pc.EBYTE} <= seen


def test_records_that_do_not_fit_are_counted_not_written(ctx):
    import ctypes as C
    text = np.frombuffer(HAND["width60"], np.uint8)
    lib = capi.lib()
    d_text = ctx.upload(text)
    d_scratch = capi.DevBuf(ctx, int(lib.palace_fasta_index_scratch_bytes(len(text))))
    d_recs = ctx.upload(np.full(7 * capi.FASTA_REC_DTYPE.itemsize, 0xA5, np.uint8))
    st = capi.FastaStatus()
    for cap in (0, 3, 6):
        capi._check(lib.palace_fasta_index(ctx.h, d_text.ptr, len(text), d_recs.ptr, cap, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
        assert int(st.n_records) == 7 and (d_recs.to_host() == 0xA5).all()
    capi._check(lib.palace_fasta_index(ctx.h, d_text.ptr, len(text), d_recs.ptr, 7, d_scratch.ptr, d_scratch.nbytes, C.byref(st)), "palace_fasta_index")
    got = d_recs.to_host().view(capi.FASTA_REC_DTYPE)
    assert int(st.n_records) == 7 and [int(x) for x in got["length"]] == [0, 1, 59, 60, 61, 303, 700]
