"""palace_final_fasta_lengths and palace_final_fasta_write (csrc/final_fasta.hip) at the C ABI, behind the index, the names and
the look-up of make_fa_from_path, byte for byte against the restatement of tests/final_fa_cases.py.  The host's part -- tokens,
headers, the paths' places -- is done here in Python; the graph is empty, so every path is written whole."""
import numpy as np
import pytest

from palace_amd import capi
from tests import final_fa_cases as fc
from tests import path_fasta_cases as pc

pytestmark = pytest.mark.gpu

IUPAC = b"ACGTRYKMBDHVSWNacgtrykmbdhvswn"
LENGTHS = (0, 1, 15, 16, 17, 4097)


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def name(n):
    return b"c_length_%d" % n


def assembly(eol, width):
    rng = np.random.default_rng(31)
    alphabet = np.frombuffer(IUPAC + b"*.-", np.uint8)
    recs = [(name(n) + (b" len=%d" % n if n % 2 else b""), alphabet[rng.integers(0, len(alphabet), size=n)].tobytes()) for n in LENGTHS]
    recs.insert(3, (b"iupac_length_30", IUPAC))
    return pc.fasta_text(recs, width, eol)


PATHS = (b"".join(name(n) + s + b" " for n in LENGTHS for s in (b"+", b"-")) + b"iupac_length_30+ iupac_length_30-\n"     # every record on both strands
         + b"zz_length_1+ " + name(16) + b"+ zz_length_2- " + name(17) + b"- zz_length_3+\n"                                # no record: first, middle, last
         + name(0) + b"+ " + name(15) + b"- " + name(0) + b"- " + name(1) + b"+\n"                                          # an empty first record: no separator behind it
         + b"zz_length_1+ " + name(0) + b"- zz_length_9-\n"                                                                 # ends empty: no text, no number
         + name(16) + b"_x+ " + name(1) + b"+\n"                                                                            # found only without its last '_' part: not found here
         + b"ref" + name(4097) + b"-ref\n"
         + b"iupac_length_30-\n"
         + b"zz_length_5+\n")                                                                                              # a last path without text


class Chain:
    def __init__(self, ctx, fasta, paths):
        self.ff = capi.FinalFasta(ctx, fasta)
        plist = fc.parse_paths(paths)
        tokens = [fc.query_of(t) for _, toks in plist for t in toks]
        path_off = np.zeros(len(plist) + 1, np.int64)
        np.cumsum([len(toks) for _, toks in plist], out=path_off[1:])
        self.codes, d_code = self.ff.resolve(tokens)
        self.lens, d_cum, d_path_off = self.ff.lengths(d_code, path_off)
        self.cum = d_cum.to_host()
        count, headers = 0, []
        for l in self.lens:
            count += l > 0
            headers.append(b"P_phage_%d_linear" % count if l > 0 else None)
        self.total, self.windows = self.ff.writer(d_code, d_cum, d_path_off, headers, self.lens)
        self.want, self.err = fc.final_fa(paths, b"", fasta, b"P", b"f.fa", b"o.fa")
        assert self.total == len(self.want)

    def check(self, cuts):
        got, intact = self.windows(cuts)
        assert intact, "bytes outside a window were written"
        if got != self.want:
            at = next((i for i, (a, b) in enumerate(zip(got, self.want)) if a != b), min(len(got), len(self.want)))
            raise AssertionError((at, got[max(0, at - 20):at + 20], self.want[max(0, at - 20):at + 20]))


@pytest.fixture(scope="module", params=[(b"\r\n", 60), (b"\n", 16), (b"\n", 100000)], ids=["crlf60", "lf16", "one_line"])
def chain(ctx, request):
    c = Chain(ctx, assembly(*request.param), PATHS)
    yield c
    c.ff.close()


def test_lengths_and_places(chain):
    seq_lens = [len(l) for l in chain.want.split(b"\n")[1::2]]
    assert [int(l) for l in chain.lens if l > 0] == seq_lens and [int(l) for l in chain.lens].count(0) == 2
    codes = [int(c) for c in chain.codes]
    assert codes.count(capi.PATH_NOT_FOUND) == 6 and sum(1 for c in codes if c >= 0 and c & capi.PATH_SECOND_TRY) == 1
    assert chain.err.count(b"Warning: Node '") == 7                                # (the second try counts as not found)
    # the first path: every record on both strands, a separator in front of each but the first that brings bytes (c_length_0 brings none)
    n_first = 2 * len(LENGTHS) + 2
    steps = np.diff(chain.cum[:n_first + 1])
    rec_len = [n for n in LENGTHS for _ in (0, 1)] + [30, 30]
    assert [int(s) for s in steps] == [n + (50 if k > 2 else 0) for k, n in enumerate(rec_len)]
    assert int(chain.lens[0]) == sum(rec_len) + 50 * (n_first - 3) and int(chain.lens[2]) == 15 + 50 + 0 + 50 + 1


def test_whole_text(chain):
    assert chain.total > 3 * 4099
    assert chain.want.count(b">") == 6 and b">P_phage_6_linear\n" in chain.want and fc.reverse_complement(IUPAC) + b"\n" in chain.want
    chain.check([])


def test_windows_of_16_and_4099_bytes_at_every_offset_modulo_16(chain):
    n = chain.total
    for size in (16, 4099):
        for s in range(16):
            chain.check([c for c in range(s, n, size) if c > 0] if size == 16 else [c for c in range(size - 16 + s, n, size)])


def test_windows_of_one_byte(chain):
    chain.check(list(range(1, chain.total)))


def test_complement_table_on_both_strands(ctx):
    fasta = b">iupac_length_30 x\n" + IUPAC[:7] + b"\n" + IUPAC[7:14] + b"\n" + IUPAC[14:21] + b"\n" + IUPAC[21:28] + b"\n" + IUPAC[28:] + b"\n>o_length_1\n@[`{~\n"
    c = Chain(ctx, fasta, b"iupac_length_30+ iupac_length_30- o_length_1-\n")
    assert c.want == b">P_phage_1_linear\n" + IUPAC + fc.SEP + b"nwsbdhvkmryacgtNWSBDHVKMRYACGT" + fc.SEP + b"~{`[@\n"
    c.check([])
    c.check(list(range(1, c.total)))
    c.ff.close()


def test_no_text_at_all(ctx):
    c = Chain(ctx, b">a_length_1\nAC\n", b"zz_length_1+\nall\nzz_length_2- zz_length_3+\n")
    assert c.total == 0 and c.want == b"" and [int(l) for l in c.lens] == [0, 0]
    c.check([])
    c.ff.close()
