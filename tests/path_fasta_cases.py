"""make_fa_from_path restated in plain Python, and the inputs of its tests (no tests here; `python -m tests.path_fasta_cases` checks
the restatement against hand-written files).

The rules are DESIGN.md 8's: the FASTA index as `samtools faidx` would build it (restated as a streaming parse: the kernels judge
every line by itself, this file walks the lines in order), the paths file's lines and tokens, the two tries of a name, the
A/C/G/T-only complement, and the records.  Nothing of the reference's script is copied: it cannot run where pysam is absent, so
parity is unpinned and these rules ARE the definition."""
import numpy as np

OK, ETEXT, ENAME, ERAGGED, EBLANK, EBYTE = range(6)
NOTHING, NOT_FOUND = -1, -2
WS = b" \t\r\n\x0b\x0c"
TILE = 4096                      # palace_amd.capi.FASTA_TILE_BYTES; the tests assert that they agree


class FastaError(Exception):
    def __init__(self, code, line):
        super().__init__(f"FASTA fault {code} at line {line}")
        self.code, self.line = code, line


def fasta_index(text: bytes):
    """-> (records, code, line): records as dicts of name, name_off, name_len, seq_off, length, line_bases, line_width in file
    order; code / line: the smallest (1-based line, code) among the text's faults, (0, 0) without one"""
    faults = []
    if text and text[:1] != b">":
        faults.append((1, ETEXT))
    recs, cur, first, prev = [], None, None, None
    pos, n, line_no = 0, len(text), 0
    while pos < n:
        line_no += 1
        e = text.find(b"\n", pos)
        term = e >= 0
        if not term:
            e = n
        line = text[pos:e]
        if line[:1] == b">":
            k = 1
            while k < len(line) and line[k:k + 1] not in (b" ", b"\t", b"\r"):
                k += 1
            if k == 1:
                faults.append((line_no, ENAME))
            cur = dict(name=line[1:k], name_off=pos + 1, name_len=k - 1, seq_off=e + 1 if term else n, length=0, line_bases=0, line_width=0)
            recs.append(cur)
            first = prev = None
        elif cur is not None:
            b = len(line) - (1 if term and line.endswith(b"\r") else 0)
            w = len(line) + (1 if term else 0)
            if any(c < 0x21 or c > 0x7e for c in line[:b]):
                faults.append((line_no, EBYTE))
            if first is None:
                first = (b, w)
                cur["line_bases"], cur["line_width"] = b, w
            elif b > 0:
                if prev[0] == 0:
                    faults.append((line_no, EBLANK))
                elif prev != first or b > first[0]:
                    faults.append((line_no, ERAGGED))
            cur["length"] += b
            prev = (b, w)
        pos = e + 1
    if faults:
        line, code = min(faults)
        return recs, code, line
    return recs, OK, 0


def sequence_of(text: bytes, rec) -> bytes:
    """a record's bases through the index arithmetic alone"""
    b, w, s = rec["line_bases"], rec["line_width"], rec["seq_off"]
    return bytes(text[s + p // b * w + p % b] for p in range(rec["length"]))


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def reverse_complement(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def path_lines(paths: bytes):
    """-> [(0-based line index, [token as split, ...])] of the lines that give a record"""
    if not paths:
        return []
    lines = paths.split(b"\n")
    if paths.endswith(b"\n"):
        lines.pop()
    out = []
    for i, line in enumerate(lines):
        if line.startswith(b"iter") or line.startswith(b"self") or line.strip(WS) == b"":
            continue
        out.append((i, line.strip(WS).split(b"\t")))
    return out


def clean(token: bytes) -> bytes:
    return token.replace(b" ", b"").strip(WS)


def shortened(name: bytes) -> bytes:
    return b"_".join(name.split(b"_")[:-1])


def resolve(token: bytes, first_of: dict):
    """a cleaned token -> NOTHING, NOT_FOUND or (record, reverse, second try)"""
    if len(token) <= 1:
        return NOTHING
    name = token[:-1] if token[-1:] in (b"+", b"-") else token
    rev = token[-1:] == b"-"
    if name in first_of:
        return first_of[name], rev, False
    short = shortened(name)
    if short and short in first_of:
        return first_of[short], rev, True
    return NOT_FOUND


def needs_second_try_line(token: bytes, first_of: dict):
    """the stdout line of an unoriented token whose own name is no record, or None"""
    if len(token) <= 1 or token[-1:] in (b"+", b"-") or token in first_of:
        return None
    return b"Contig not found: " + shortened(token) + b"\n"


class MissingContig(Exception):
    def __init__(self, line, token, stdout):
        super().__init__(f"line {line}: {token!r}")
        self.line, self.token, self.stdout = line, token, stdout


def first_records(recs):
    first_of = {}
    for i, r in enumerate(recs):
        first_of.setdefault(r["name"], i)
    return first_of


def make_fa(fasta: bytes, paths: bytes, mode: bytes):
    """-> (output text, stdout); raises FastaError or MissingContig (whose stdout is what was printed up to the failing token)"""
    recs, code, line = fasta_index(fasta)
    stdout = b"make_fa_from_path.py running\n"
    if code:
        raise FastaError(code, line)
    first_of = first_records(recs)
    seqs = {}
    plan = []
    for idx, tokens in path_lines(paths):
        parts = []
        for tok in tokens:
            c = clean(tok)
            note = needs_second_try_line(c, first_of)
            if note:
                stdout += note
            r = resolve(c, first_of)
            if r == NOT_FOUND:
                raise MissingContig(idx + 1, c, stdout)
            if r != NOTHING:
                if r[0] not in seqs:
                    seqs[r[0]] = sequence_of(fasta, recs[r[0]])
                parts.append(reverse_complement(seqs[r[0]]) if r[1] else seqs[r[0]])
        plan.append((idx, tokens, b"".join(parts)))
    out = []
    for idx, tokens, seq in plan:
        header = b"res_%d_%d" % (idx + 1, len(seq)) if mode == b"0" else b"".join(tokens)
        out.append(b">" + header + b"\n" + seq + b"\n")
    return b"".join(out), stdout


# ---- builders ---------------------------------------------------------------------------------------------------------------------

ALPHABET = np.frombuffer(b"ACGTacgtNnRy*", dtype=np.uint8)


def random_seq(rng, n: int) -> bytes:
    return ALPHABET[rng.integers(0, len(ALPHABET), size=n)].tobytes()


def fasta_text(records, width: int, eol: bytes = b"\n", final_eol: bool = True) -> bytes:
    """records: [(header text behind '>', sequence)] folded at `width` bases"""
    out = []
    for head, seq in records:
        out.append(b">" + head + eol)
        for k in range(0, len(seq), width):
            out.append(seq[k:k + width] + eol)
    text = b"".join(out)
    return text if final_eol else text[:len(text) - len(eol)]


def hand_fastas(rng):
    """{case: FASTA text} of the well-formed hand cases of the index test"""
    def recs(lengths, prefix=b"c"):
        return [(prefix + b"%d" % i, random_seq(rng, n)) for i, n in enumerate(lengths)]
    cases = {}
    for w in (1, 15, 16, 17, 60):
        cases[f"width{w}"] = fasta_text(recs([0, 1, w - 1, w, w + 1, 5 * w + 3, 700]), w)
    # ">c0\n" is 4 bytes: a first line of TILE - 5 bases has its LF on the tile's last byte, one of TILE - 4 on the next tile's first
    cases["lf_on_tile_last_byte"] = fasta_text(recs([3 * (TILE - 5) + 7]), TILE - 5)
    cases["lf_on_tile_first_byte"] = fasta_text(recs([3 * (TILE - 4) + 7]), TILE - 4)
    cases["last_line_full_width"] = fasta_text(recs([120, 60, 180]), 60)
    cases["no_final_lf"] = fasta_text(recs([100, 47]), 60, final_eol=False)
    cases["no_final_lf_full_line"] = fasta_text(recs([100, 120]), 60, final_eol=False)
    cases["crlf"] = fasta_text(recs([0, 1, 59, 60, 61, 500]), 60, eol=b"\r\n")
    cases["crlf_no_final"] = fasta_text(recs([61, 75]), 60, eol=b"\r\n", final_eol=False)
    cases["empty_records"] = fasta_text([(b"a", random_seq(rng, 70)), (b"empty1", b""), (b"b", random_seq(rng, 10)), (b"empty2", b"")], 60)
    cases["header_only_no_lf"] = b">a\nACGT\n>last"
    cases["one_base"] = b">x\nA\n"
    cases["description"] = fasta_text([(b"ctg1 length=70 cov=3.5", random_seq(rng, 70)), (b"ctg2\tflag", random_seq(rng, 5)), (b"ctg3 ", b"AC")], 60)
    cases["duplicates"] = fasta_text([(b"dup", b"AAAA"), (b"other", b"CC"), (b"dup", b"GGGGGG"), (b"dup x", b"T")], 60)
    cases["three_tiles"] = fasta_text(recs([3 * TILE + 1234, 5]), 70)
    cases["one_long_line"] = fasta_text(recs([2 * TILE + 77, 9]), 1 << 20)
    cases["many_in_one_tile"] = fasta_text([(b"%d" % i, random_seq(rng, 1 + i % 7)) for i in range(300)], 60)
    cases["blank_tail"] = b">a\nACGT\nAC\n\n\n>b\n\n>c\nAA\n\n"
    cases["empty"] = b""
    return cases


def malformed_fastas(rng):
    """{case: (FASTA text, code, 1-based line)}: each fault alone"""
    good = [(b"r%d" % i, random_seq(rng, n)) for i, n in enumerate([130, 300, 61])]
    lines = fasta_text(good, 60).split(b"\n")[:-1]

    def text_of(ls):
        return b"\n".join(ls) + b"\n"
    cases = {}
    ragged = list(lines)
    ragged[2] = ragged[2][:-3]                                      # the first record's second line of three: short, a line follows
    cases["ragged_middle"] = (text_of(ragged), ERAGGED, 4)
    longer = list(lines)
    longer[3] = longer[3] + b"A" * 60                               # the first record's last line: longer than the first
    cases["last_line_longer"] = (text_of(longer), ERAGGED, 4)
    # a ragged line that ends exactly at a tile boundary: the line behind it, which is at fault, begins the next tile
    w = 64
    body = [random_seq(rng, w) for _ in range(200)]
    pre = b">t\n"
    k = (TILE - 1 - len(pre)) // (w + 1) + 1                        # lines that end inside the first tile
    short = TILE - len(pre) - (k - 1) * (w + 1) - 1                 # ... the k-th cut so that its LF is the tile's last byte
    assert 0 < short < w
    body[k - 1] = body[k - 1][:short]
    t = pre + text_of(body)
    assert t[TILE - 1:TILE] == b"\n" and t[TILE - 2:TILE - 1] != b"\n"
    cases["ragged_at_tile_boundary"] = (t, ERAGGED, k + 2)
    blank = list(lines)
    blank.insert(2, b"")
    cases["blank_inside"] = (text_of(blank), EBLANK, 4)
    cases["blank_first_line"] = (b">a\n\nACGT\n", EBLANK, 3)
    cases["text_before"] = (b"ACGT\n" + text_of(lines), ETEXT, 1)
    cases["blank_before"] = (b"\n" + text_of(lines), ETEXT, 1)
    noname = list(lines)
    noname[4] = b"> r1"
    cases["empty_name"] = (text_of(noname), ENAME, 5)
    cases["empty_name_at_end"] = (text_of(lines) + b">", ENAME, len(lines) + 1)
    tab = list(lines)
    tab[6] = tab[6][:10] + b"\t" + tab[6][11:]
    cases["tab_in_sequence"] = (text_of(tab), EBYTE, 7)
    cr = list(lines)
    cr[1] = cr[1][:5] + b"\r" + cr[1][6:]
    cases["cr_inside_line"] = (text_of(cr), EBYTE, 2)
    cases["cr_at_end_without_lf"] = (b">a\nACGT\r", EBYTE, 2)
    mixed = [l + b"\r" if i == 2 else l for i, l in enumerate(lines)]
    cases["one_crlf_line"] = (text_of(mixed), ERAGGED, 4)           # same bases, another width: the line behind it is at fault
    two = list(ragged)
    two[6] = two[6][:10] + b" " + two[6][11:]
    cases["two_faults_first_wins"] = (text_of(two), ERAGGED, 4)
    return cases


def random_fasta(rng, n_records: int, max_len: int = 3000) -> bytes:
    out = []
    for i in range(n_records):
        w = int(rng.integers(1, 121))
        n = int(rng.integers(0, max_len + 1))
        eol = b"\r\n" if rng.integers(0, 8) == 0 else b"\n"
        out.append(fasta_text([(b"NODE_%d_length_%d" % (i, n) + (b" d" if i % 5 == 0 else b""), random_seq(rng, n))], w, eol))
        if rng.integers(0, 10) == 0 and n:
            out.append(eol)                                         # blank lines behind a record's last line
    return b"".join(out)


def chain_fasta(rng, line_bases: int = 60):
    """the assembly of the chain tests: contigs of lengths 0, 1, line_bases - 1, line_bases, line_bases + 1 and 5000, a duplicate
    name, names with '_' parts -> (text, names)"""
    lengths = [0, 1, line_bases - 1, line_bases, line_bases + 1, 5000, 333, 77]
    names = [b"NODE_%d" % i for i in range(len(lengths))]
    records = [(nm, random_seq(rng, n)) for nm, n in zip(names, lengths)]
    records.insert(4, (b"NODE_6", random_seq(rng, 21)))             # a later NODE_6 exists: this one, the first, is used
    records.append((b"plain", random_seq(rng, 40)))
    records.append((b"x", random_seq(rng, 12)))                     # a one-letter name: its token contributes nothing
    return fasta_text(records, line_bases), names


CHAIN_PATHS = (b"NODE_5+\tNODE_1-\tNODE_2+\n"
               b"iter 3\n"
               b"NODE_3-\tNODE_4-\tNODE_0+\tNODE_5-\n"
               b"self loop\n"
               b"\n"
               b"NODE_6+\tNODE_6-\n"                                # the duplicate name: the first record
               b"NODE_2_7+\tNODE_3_part-\tplain_1\tplain\n"   # second tries, oriented and not
               b"x\t+\t-\tx+\tNODE_1+\t\tN ODE_ 4+ \t\n"            # nothing, nothing, nothing, a record named x, ..., an empty token, spaces
               b" \t \r\n"                                          # blank after stripping
               b"NODE_0+\n"                                         # an empty sequence
               b"NODE_7-")                                          # no LF at the end


def hand_checks():
    """the restatement against files written by hand"""
    fa = b">a desc\nACGTN\nacg\n>b\n>c_1\nRY*nT\n>a\nTTTT\n"
    recs, code, line = fasta_index(fa)
    assert (code, line) == (OK, 0)
    assert [(r["name"], r["name_off"], r["seq_off"], r["length"], r["line_bases"], r["line_width"]) for r in recs] == \
        [(b"a", 1, 8, 8, 5, 6), (b"b", 19, 21, 0, 0, 0), (b"c_1", 22, 26, 5, 5, 6), (b"a", 33, 35, 4, 4, 5)]
    assert sequence_of(fa, recs[0]) == b"ACGTNacg" and reverse_complement(b"ACGTNacgRY*") == b"*YRcgtNACGT"
    paths = b"a+\tc_1-\niter 1\n\nself\nc_1_9\tb+\t \ta -\n\t\nq\tx\n"
    out, stdout = make_fa(fa, paths, b"0")
    assert out == b">res_1_13\nACGTNacgAn*YR\n>res_5_13\nRY*nTcgtNACGT\n>res_7_0\n\n", out
    assert stdout == b"make_fa_from_path.py running\nContig not found: c_1\n"
    out1, _ = make_fa(fa, paths, b"1")
    assert out1 == b">a+c_1-\nACGTNacgAn*YR\n>c_1_9b+ a -\nRY*nTcgtNACGT\n>qx\n\n", out1
    try:
        make_fa(fa, b"a+\nzz_1\tnope_1_2+\n", b"0")
        raise AssertionError("a missing contig must raise")
    except MissingContig as m:
        assert (m.line, m.token, m.stdout) == (2, b"zz_1", b"make_fa_from_path.py running\nContig not found: zz\n")
    crlf = b">k\r\nAC\r\nG\r\n"
    recs, code, line = fasta_index(crlf)
    assert code == OK and (recs[0]["name"], recs[0]["seq_off"], recs[0]["length"], recs[0]["line_bases"], recs[0]["line_width"]) == (b"k", 4, 3, 2, 4)
    assert sequence_of(crlf, recs[0]) == b"ACG"
    assert fasta_index(b">a\nAC\nA\nAC\n")[1:] == (ERAGGED, 4) and fasta_index(b">a\nAC\n\nAC\n")[1:] == (EBLANK, 4)
    assert fasta_index(b"x\n>a\n")[1:] == (ETEXT, 1) and fasta_index(b">a\n>\n")[1:] == (ENAME, 2) and fasta_index(b">a\nA C\n")[1:] == (EBYTE, 2)
    assert path_lines(b"a\tb") == [(0, [b"a", b"b"])] and path_lines(b"") == [] and path_lines(b"\n") == []
    rng = np.random.default_rng(3)
    for name, (text, code, line) in malformed_fastas(rng).items():
        assert fasta_index(text)[1:] == (code, line), (name, fasta_index(text)[1:], code, line)
    for name, text in hand_fastas(rng).items():
        recs, code, line = fasta_index(text)
        assert code == OK, (name, code, line)
    text, _ = chain_fasta(rng)
    out, stdout = make_fa(text, CHAIN_PATHS, b"0")
    assert out.count(b">") == 7 and stdout.count(b"Contig not found") == 1 and b">res_11_77\n" in out and b">res_10_0\n\n" in out


if __name__ == "__main__":
    hand_checks()
    print("path_fasta_cases: the restatement agrees with the hand-written files")
