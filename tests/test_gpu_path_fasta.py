"""The ABI chain behind make_fa_from_path (csrc/path_fasta.hip): palace_fasta_index -> palace_fasta_names_create ->
palace_path_resolve -> palace_path_fasta_lengths -> palace_path_fasta_write, byte for byte against the Python restatement of
tests/path_fasta_cases.py.  The host's part of the executable -- tokens, headers, the paths' places -- is done here in Python."""
import numpy as np
import pytest

from palace_amd import capi, synth
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def want_code(r):
    if r in (pc.NOTHING, pc.NOT_FOUND):
        return r
    return (r[0] << 2) | (capi.PATH_SECOND_TRY if r[2] else 0) | (capi.PATH_REVERSE if r[1] else 0)


class Chain:
    """one FASTA and one paths text through the device, up to the writer"""

    def __init__(self, ctx, fasta, paths, mode):
        self.pf = capi.PathFasta(ctx, fasta)
        recs, code, _ = pc.fasta_index(fasta)
        assert code == pc.OK
        self.first_of = pc.first_records(recs)
        lines = pc.path_lines(paths)
        tokens = [pc.clean(t) for _, toks in lines for t in toks]
        path_off = np.zeros(len(lines) + 1, np.int64)
        np.cumsum([len(toks) for _, toks in lines], out=path_off[1:])
        self.codes, d_code = self.pf.resolve(tokens)
        assert [int(c) for c in self.codes] == [want_code(pc.resolve(t, self.first_of)) for t in tokens]
        self.lens, d_cum, d_path_off = self.pf.lengths(d_code, path_off)
        headers = [b"res_%d_%d" % (idx + 1, int(l)) if mode == b"0" else b"".join(toks) for (idx, toks), l in zip(lines, self.lens)]
        self.total, self.windows = self.pf.writer(d_code, d_cum, d_path_off, headers, self.lens)
        self.want, _ = pc.make_fa(fasta, paths, mode)
        assert self.total == len(self.want)

    def check(self, cuts):
        got, intact = self.windows(cuts)
        assert intact, "bytes outside a window were written"
        if got != self.want:
            at = next(i for i, (a, b) in enumerate(zip(got, self.want)) if a != b)
            raise AssertionError((at, got[max(0, at - 20):at + 20], self.want[max(0, at - 20):at + 20]))


@pytest.fixture(scope="module")
def chain(ctx):
    fasta, _ = pc.chain_fasta(synth.rng_for(21))
    c = Chain(ctx, fasta, pc.CHAIN_PATHS, b"0")
    yield c
    c.pf.close()


def test_resolution_and_lengths(chain):
    codes = [int(c) for c in chain.codes]
    assert codes.count(pc.NOTHING) >= 4 and pc.NOT_FOUND not in codes
    assert sum(1 for c in codes if c >= 0 and c & capi.PATH_SECOND_TRY) == 3          # two oriented, one not
    assert sum(1 for c in codes if c >= 0 and c & capi.PATH_REVERSE) >= 5
    assert sorted({int(l) for l in chain.lens})[0] == 0 and max(int(l) for l in chain.lens) > 5000
    dup = chain.pf.duplicates()
    assert dup.sum() == 1 and dup[7] == 1                                            # the second NODE_6


def test_duplicate_name_is_the_first_record(ctx, chain):
    codes, _ = chain.pf.resolve([b"NODE_6+", b"NODE_6_x-", b"NODE_6"])
    assert [int(c) >> 2 for c in codes] == [4, 4, 4]
    assert [int(c) & 3 for c in codes] == [0, capi.PATH_SECOND_TRY | capi.PATH_REVERSE, 0]


def test_tokens_that_are_not_found_or_nothing(chain):
    tokens = [b"nowhere+", b"NODE_99", b"NODE_1_a_b+", b"_NODE_1+", b"NODE_1_", b"", b"+", b"-", b"x", b"N", b"NODE_1", b"ODE_1+", b"NODE_1++", b"NODE_1+-"]
    codes, _ = chain.pf.resolve(tokens)
    assert [int(c) for c in codes] == [want_code(pc.resolve(t, chain.first_of)) for t in tokens]
    assert [int(c) for c in codes[:5]] == [pc.NOT_FOUND] * 4 + [(1 << 2) | capi.PATH_SECOND_TRY]
    assert [int(c) for c in codes[5:10]] == [pc.NOTHING] * 5


def test_whole_and_in_windows(chain):
    n = chain.total
    assert n > 10000
    chain.check([])
    for step in (16, 17, 4096):
        chain.check(list(range(step, n, step)))
    rng = synth.rng_for(22)
    for k in (3, 40):
        cuts = sorted(int(c) for c in rng.integers(0, n + 1, size=k))
        chain.check(sorted(cuts + cuts[:2]))                                         # (empty windows among them)


def test_one_byte_windows(chain):
    chain.check(list(range(1, chain.total)))


def test_mode_with_joined_tokens_as_headers(ctx):
    fasta, _ = pc.chain_fasta(synth.rng_for(21), line_bases=17)
    c = Chain(ctx, fasta, pc.CHAIN_PATHS, b"1")
    assert b">x+-x+NODE_1+N ODE_ 4+\n" in c.want
    c.check([])
    c.check(list(range(5, c.total, 5)))
    c.pf.close()


@pytest.mark.parametrize("eol,width", [(b"\n", 1), (b"\r\n", 60), (b"\n", 16), (b"\n", 100000)])
def test_line_shapes(ctx, eol, width):
    rng = synth.rng_for(23)
    recs = [(b"c_%d" % i, pc.random_seq(rng, n)) for i, n in enumerate([0, 1, 15, 16, 17, 31, 32, 33, 600, 5000])]
    fasta = pc.fasta_text(recs, width, eol)
    paths = b"".join(b"c_%d%s\t" % (i, s) for i in range(10) for s in (b"+", b"-")) + b"\n" + b"c_9-\nc_8-\tc_8-\n"
    c = Chain(ctx, fasta, paths, b"0")
    c.check([])
    c.check(list(range(33, c.total, 33)))
    c.pf.close()


def test_one_long_path_and_many_short_ones(ctx):
    rng = synth.rng_for(24)
    fasta = pc.random_fasta(rng, 200, max_len=400)
    recs, code, _ = pc.fasta_index(fasta)
    assert code == pc.OK
    pick = lambda: recs[int(rng.integers(0, 200))]["name"] + (b"+", b"-")[int(rng.integers(0, 2))]
    paths = b"\t".join(pick() for _ in range(1000)) + b"\n" + b"".join(pick() + b"\n" for _ in range(1000))
    c = Chain(ctx, fasta, paths, b"0")
    assert len(c.lens) == 1001 and int(c.lens[0]) > 100000
    c.check([])
    c.check(list(range(4099, c.total, 4099)))
    c.pf.close()


def test_no_paths_no_bytes(ctx):
    c = Chain(ctx, b">a\nAC\n", b"iter 0\n\nself\n", b"0")
    assert c.total == 0 and c.want == b""
    c.check([])
    c.pf.close()
