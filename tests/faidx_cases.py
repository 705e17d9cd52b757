"""faidx restated in plain Python, and the inputs of its tests (no tests here; `python -m tests.faidx_cases` checks the restatement
against hand-written texts).

The rules are DESIGN.md 8's.  samtools, htslib, pyfaidx, pysam and Biopython are all absent where this was written: parity with
`samtools faidx` is UNPINNED and these rules ARE the definition; tests/test_host_faidx_rules.py pins them to a hand-typed catalogue.
The index is tests/path_fasta_cases.py's, imported unchanged."""

from tests.path_fasta_cases import fasta_index, fasta_text, first_records, random_seq, sequence_of

MAX_DIGITS = 18
FAULT_TEXT = {1: b"text before the first '>'", 2: b"a header line without a name",
              3: b"a sequence line behind a line of another length than the record's first (only a record's last line may be shorter)",
              4: b"a sequence line behind a blank line of its record", 5: b"a sequence byte outside 0x21-0x7E"}

# Biopython's ambiguous-DNA complement in either case; every other byte stays
_COMP = bytes.maketrans(b"ACGTRYKMBVDHacgtrykmbvdh", b"TGCAYRMKVBHDtgcayrmkvbhd")


def reverse_complement(seq: bytes) -> bytes:
    return seq.translate(_COMP)[::-1]


def number(s: bytes):
    """digits in which ',' is ignored: at least one digit, at most 18 -> the value, or None"""
    d = s.replace(b",", b"")
    if not d or len(d) > MAX_DIGITS or any(c not in b"0123456789" for c in d):
        return None
    return int(d)


def parse_range(s: bytes):
    """the part behind the colon -> (B, E) 1-based as written (B = 0 counted as 1, a missing E None), or None"""
    if not s or s == b"-":
        return None
    if s[:1] == b"-":
        b, e = 1, number(s[1:])
        if e is None:
            return None
    else:
        head, dash, tail = s.partition(b"-")
        b = number(head)
        if b is None:
            return None
        b = max(b, 1)
        e = None
        if dash and tail:
            e = number(tail)
            if e is None:
                return None
    if e is not None and e < b:
        return None
    return b, e


def resolve(region: bytes, recs, first_of):
    """-> (rec, beg 0-based, len), (-1, 0, 0) for a region that fails"""
    if region in first_of:
        r = first_of[region]
        return r, 0, recs[r]["length"]
    cut = region.rfind(b":")
    if cut < 0 or region[:cut] not in first_of:
        return -1, 0, 0
    rng = parse_range(region[cut + 1:])
    if rng is None:
        return -1, 0, 0
    r = first_of[region[:cut]]
    n = recs[r]["length"]
    b, e = rng
    if b > n:
        return r, n, 0
    e = n if e is None else min(e, n)
    return r, b - 1, e - (b - 1)


def strand_mark(mark: str, reverse: bool) -> bytes:
    if mark == "no":
        return b""
    if mark == "sign":
        return b"(-)" if reverse else b"(+)"
    return b"/rc" if reverse else b""


def region_text(header: bytes, seq: bytes, n: int) -> bytes:
    return b">" + header + b"\n" + b"".join(seq[k:k + n] + b"\n" for k in range(0, len(seq), n))


def fetch(fasta: bytes, regions, n: int = 60, reverse: bool = False, mark: str = "rc", keep_going: bool = False):
    """-> (stdout, stderr, exit status) of `faidx [-n n] [-i] [--mark-strand mark] [-c] file regions...` on a well-formed FASTA"""
    recs, code, line = fasta_index(fasta)
    assert code == 0, (code, line)
    first_of = first_records(recs)
    out, err = [], []
    for region in regions:
        r, beg, ln = resolve(region, recs, first_of)
        if r < 0:
            err.append(b"[faidx] Failed to fetch sequence in " + region + b"\n")
            if not keep_going:
                return b"", err[-1], 1
            continue
        if ln == 0:
            err.append(b"[faidx] Zero length sequence: " + region + b"\n")
        seq = sequence_of(fasta, recs[r])[beg:beg + ln]
        out.append(region_text(region + strand_mark(mark, reverse), reverse_complement(seq) if reverse else seq, n))
    return b"".join(out), b"".join(err), 0


def region_file_lines(text: bytes):
    """the regions of a -r file: its lines, a trailing CR stripped; a blank line is a region"""
    lines = text.split(b"\n")
    if text.endswith(b"\n") or not text:
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def fai_rows(fasta: bytes):
    """-> (the `.fai` text, [1-based record numbers left out because an earlier record has their name]) of a well-formed FASTA"""
    recs, code, line = fasta_index(fasta)
    assert code == 0, (code, line)
    first_of = first_records(recs)
    rows, dropped = [], []
    for i, r in enumerate(recs):
        if first_of[r["name"]] != i:
            dropped.append(i + 1)
            continue
        rows.append(b"%s\t%d\t%d\t%d\t%d\n" % (r["name"], r["length"], r["seq_off"], r["line_bases"], r["line_width"]))
    return b"".join(rows), dropped


def plan(resolved, header_lens, n: int):
    """the regions' places in the output text: len(resolved) + 1 offsets"""
    off = [0]
    for (r, _, ln), h in zip(resolved, header_lens):
        off.append(off[-1] + (0 if r < 0 else 2 + h + ln + (ln + n - 1) // n))
    return off


def abi_text(fasta: bytes, recs, resolved, headers, n: int, reverse: bool) -> bytes:
    """the output text of palace_faidx_write for resolved regions and the headers given"""
    out = []
    for (r, beg, ln), h in zip(resolved, headers):
        if r < 0:
            continue
        seq = sequence_of(fasta, recs[r])[beg:beg + ln]
        out.append(region_text(h, reverse_complement(seq) if reverse else seq, n))
    return b"".join(out)


# ---- the catalogue's FASTA and region strings ---------------------------------------------------------------------------------------

CATALOGUE_FASTA = (b">chr1 the first\nACGTACGTAC\nGTACGTACGT\nACGTA\n"          # 25 bases in lines of 10
                   b">a:b\nAAAACCCCGG\n"                                        # a name with ':' -- 10 bases
                   b">a:b:2-3\nTTTT\n"                                          # a name that reads as a region of a:b
                   b">chr1\nGGGG\n"                                             # the name again: never found
                   b">ambi\nRYKMBVDHSWN\nacgtn*\n"                              # 17 bases in lines of 11
                   b">empty\n"
                   b">p|q|r\nACGTACGTACGT\n")

# every region string the grammar is asked about, in the self-test and at the ABI
GRAMMAR_REGIONS = [
    b"chr1", b"chr1:3-12", b"chr1:-4", b"chr1:21-", b"chr1:22", b"chr1:1,0-1,2", b"chr1:0-3", b"chr1:0", b"chr1:20-99", b"chr1:25-25", b"chr1:25-",
    b"chr1:26", b"chr1:26-30", b"chr1:1000000-", b"chr1:5-4", b"chr1:0-0", b"chr1:-0", b"chr1:1-1", b"a:b", b"a:b:2-3", b"a:b:2-4", b"a:b:1",
    b"a", b"a:", b"a:b:", b"chr1:", b"chr1:-", b"chr1:,", b"chr1:,-5", b"chr1:1-,", b"chr1:1,,2-3", b"chr1:,1,", b"chr1:3-12x", b"chr1:x", b"chr1:3--4",
    b"chr1:3-4-5", b"chr1: 3", b"chr1:+3", b"chr1:3-4 ", b"chr2", b"chr2:1-5", b"chr1 ", b"CHR1", b"{chr1}:1-5", b"{a:b}:1-5", b"empty", b"empty:1-5",
    b"empty:1", b"empty:0", b"p|q|r", b"p|q|r:2-3", b"ambi:1-11", b"ambi:12-", b"chr1:000000000000000001-000000000000000002",
    b"chr1:123456789012345678", b"chr1:1-123456789012345678", b"chr1:1234567890123456789", b"chr1:1-1234567890123456789",
    b"chr1:0000000000000000001", b"chr1:1,234,567,890,123,456,789", b":", b":1-2", b"::", b"-5", b"1-5", b"chr1:1-5:", b"chr1:chr1", b"chr1:chr1:2-3",
]


def synthetic_assembly(rng, n_records: int, max_len: int = 400):
    """a FASTA of NODE_<i>_length_<n> records in lines of 60, and its names"""
    records = [(b"NODE_%d_length_%d" % (i, n), random_seq(rng, n)) for i, n in enumerate(rng.integers(1, max_len + 1, size=n_records))]
    return fasta_text(records, 60), [h for h, _ in records]


def hand_checks():
    """the restatement against texts written by hand"""
    fa = CATALOGUE_FASTA
    assert fetch(fa, [b"chr1:3-12"]) == (b">chr1:3-12\nGTACGTACGT\n", b"", 0)
    assert fetch(fa, [b"chr1"], n=10)[0] == b">chr1\nACGTACGTAC\nGTACGTACGT\nACGTA\n"
    assert fetch(fa, [b"ambi"], reverse=True)[0] == b">ambi/rc\n*nacgtNWSDHBVKMRY\n"
    assert fetch(fa, [b"chr1:30"]) == (b">chr1:30\n", b"[faidx] Zero length sequence: chr1:30\n", 0)
    assert fetch(fa, [b"chr1:1-2", b"nope", b"chr1:5-4"]) == (b"", b"[faidx] Failed to fetch sequence in nope\n", 1)
    assert fetch(fa, [b"chr1:1-2", b"nope", b"chr1:3"], n=100, keep_going=True)[::2] == (b">chr1:1-2\nAC\n>chr1:3\nGTACGTACGTACGTACGTACGTA\n", 0)
    recs, _, _ = fasta_index(fa)
    fo = first_records(recs)
    assert resolve(b"a:b:2-3", recs, fo) == (2, 0, 4) and resolve(b"a:b:2-4", recs, fo) == (1, 1, 3) and resolve(b"chr1:0-0", recs, fo) == (-1, 0, 0)
    assert region_file_lines(b"a\r\n\nb") == [b"a", b"", b"b"] and region_file_lines(b"") == [] and region_file_lines(b"\n") == [b""]
    assert fai_rows(fa) == (b"chr1\t25\t16\t10\t11\na:b\t10\t49\t10\t11\na:b:2-3\t4\t69\t4\t5\nambi\t17\t91\t11\t12\nempty\t0\t117\t0\t0\np|q|r\t12\t124\t12\t13\n", [4])
    assert plan([(0, 0, 25), (-1, 0, 0), (0, 5, 0)], [4, 9, 3], 10) == [0, 34, 34, 39]


if __name__ == "__main__":
    hand_checks()
    print("faidx_cases: the restatement agrees with the hand-written texts")
