"""split_fastg restated on bytes, the `.fai` rows of its two files, and the inputs of its tests (no tests here;
`python -m tests.split_fastg_cases` checks the restatement against hand-written files).

The rules are DESIGN.md 8's.  The record rule is pinned: tests/golden/split_fastg_cases.npz holds what the reference's script
wrote for the inputs of golden_inputs(), and tests/test_split_fastg_restatement.py holds this file to those bytes.  The grammar
is the FASTA index's (tests/path_fasta_cases.fasta_index) minus the faults below; the `.fai` rows are the documented five columns
(samtools is absent: unpinned)."""
import numpy as np

from tests import path_fasta_cases as pc

EPLUS, EHIGH, ECR, ENOLF, EEMPTY, ENONAME, EBASE = range(6, 13)
_RC = bytes.maketrans(b"ACGTacgt", b"TGCATGCA")
BASES = frozenset(b"ACGTacgt")


class FastgError(Exception):
    def __init__(self, code, line):
        super().__init__(f"FASTG fault {code} at line {line}")
        self.code, self.line = code, line


def derive_name(line: bytes):
    """a header line without its LF (and without a CR directly before it), '>' included -> (name or None when V is empty, primed)"""
    t = line[1:].split(b" ", 1)[0]
    u = t[:-1]
    v = u
    for k, c in enumerate(u):
        if c in b":,":
            v = u[:k]
            break
    if not v:
        return None, False
    return (v[:-1], True) if v.endswith(b"'") else (v, False)


def records(text: bytes):
    """-> ([(name, primed, sequence bytes as they lie, 1-based line of the header)], faults as (line, code)) of a text that ends in LF"""
    faults, recs = [], []
    if not text:
        return recs, [(1, EEMPTY)]
    lines = text.split(b"\n")
    last = lines.pop()                                   # b"" when the text ends in LF
    if last:
        lines.append(last)
        faults.append((len(lines), ENOLF))
    cur = None
    for no, raw in enumerate(lines, 1):
        ended = no < len(lines) or not last              # the line has its LF
        line = raw[:-1] if ended and raw.endswith(b"\r") else raw
        if raw[:1] == b">":
            if any(c >= 0x80 for c in raw):
                faults.append((no, EHIGH))
            if b"\r" in line:
                faults.append((no, ECR))
            name, primed = derive_name(line)
            if name is None:
                faults.append((no, ENONAME))
            cur = [name, primed, [], no]
            recs.append(cur)
        elif cur is not None:
            if raw[:1] in (b"+", b"@"):
                faults.append((no, EPLUS))
            if cur[1] and any(c not in BASES for c in line):
                faults.append((no, EBASE))
            cur[2].append(line)
    return [(n, p, b"".join(s), no) for n, p, s, no in recs], faults


def verdict(text: bytes):
    """-> (code, line): the smallest (line, code) among the index's faults and the FASTG ones, (0, 0) without one"""
    _, faults = records(text)
    _, code, line = pc.fasta_index(text)
    if code:
        faults.append((line, code))
    if not faults:
        return 0, 0
    line, code = min(faults)
    return code, line


def new_verdict(text: bytes):
    """the FASTG faults alone, as palace_fastg_derive reports them"""
    _, faults = records(text)
    if not faults:
        return 0, 0
    line, code = min(faults)
    return code, line


def kept_records(text: bytes):
    """-> [(record index, name, output sequence)] of the records that are written"""
    recs, _ = records(text)
    seen, out = set(), []
    for i, (name, primed, seq, _) in enumerate(recs):
        if name in seen:
            continue
        seen.add(name)
        out.append((i, name, seq.upper().translate(_RC)[::-1] if primed else seq))
    return out


def split_fastg(text: bytes) -> bytes:
    code, line = verdict(text)
    if code:
        raise FastgError(code, line)
    return b"".join(b">" + name + b"\n" + seq + b"\n" for _, name, seq in kept_records(text))


def fai_rows(rows) -> bytes:
    return b"".join(b"%s\t%d\t%d\t%d\t%d\n" % r for r in rows)


def output_fai(text: bytes) -> bytes:
    """<output>.fai: name, L, offset, L, L + 1 per kept record; 0 for both line fields of a record without bases"""
    rows, at = [], 0
    for _, name, seq in kept_records(text):
        n = len(seq)
        rows.append((name, n, at + len(name) + 2, n, n + 1 if n else 0))
        at += len(name) + n + 3
    return fai_rows(rows)


def graph_fai(text: bytes):
    """<graph>.fai from the FASTG's own index records -> (rows, names of the records left out because an earlier one has their
    whole name)"""
    recs, code, _ = pc.fasta_index(text)
    assert code == pc.OK
    seen, rows, left_out = set(), [], []
    for r in recs:
        if r["name"] in seen:
            left_out.append(r["name"])
            continue
        seen.add(r["name"])
        rows.append((r["name"], r["length"], r["seq_off"], r["line_bases"], r["line_width"]))
    return fai_rows(rows), left_out


# ---- builders ---------------------------------------------------------------------------------------------------------------------

def dna(rng, n: int, alphabet: bytes = b"ACGT") -> bytes:
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def fold(head: bytes, seq: bytes, width: int, eol: bytes = b"\n") -> bytes:
    return b">" + head + eol + b"".join(seq[k:k + width] + eol for k in range(0, len(seq), width))


def edge(i: int, n: int) -> bytes:
    return b"EDGE_%d_length_%d_cov_%d.5" % (i, n, 3 + i % 7)


def spades(rng, lengths, width: int = 60, eol: bytes = b"\n", primed_first=()) -> bytes:
    """both strands of every edge, links to the neighbours, `width`-base lines; the edges of primed_first have the primed record
    ahead of the forward one"""
    names = [edge(i + 1, n) for i, n in enumerate(lengths)]
    out = []
    for i, n in enumerate(lengths):
        seq = dna(rng, n)
        nxt, prv = names[(i + 1) % len(names)], names[i - 1]
        fwd = fold(names[i] + (b":" + nxt + b"," + prv + b"';" if i % 3 else b";"), seq, width, eol)
        rev = fold(names[i] + b"'" + (b":" + prv + b"';" if i % 2 else b";"), pc.reverse_complement(seq), width, eol)
        out += [rev, fwd] if i in primed_first else [fwd, rev]
    return b"".join(out)


LENGTHS = [0, 1, 15, 16, 17, 59, 60, 61, 4095, 4096, 4097, 10007]


def golden_inputs():
    """{case: FASTG text inside the grammar}: what tests/golden/make_split_fastg_golden.py runs the reference's script on"""
    rng = np.random.default_rng(1812)
    cases = {}
    cases["spades60"] = spades(rng, LENGTHS, 60, primed_first=(2, 7))
    cases["spades70_crlf"] = spades(rng, [0, 1, 69, 70, 71, 700], 70, eol=b"\r\n", primed_first=(1,))
    cases["width1"] = spades(rng, [0, 1, 2, 17], 1)
    cases["primed_first_lower"] = (b">EDGE_1_length_8_cov_2';\nacgtACGT\n>EDGE_1_length_8_cov_2:EDGE_1_length_8_cov_2';\nNNNNnnnn\n"
                                   b">EDGE_2_length_4_cov_1;\nacNn\n>EDGE_2_length_4_cov_1';\nacgt\n")
    cases["three_of_one_name"] = (b">E_1;\nAAAA\n>E_2;\nCC\n>E_1';\nGGGGGG\n>E_1:E_2;\nT\n>E_2':E_1;\nGG\n")
    cases["quirks"] = (b">EDGE_3_length_4_cov_9 extra:words;\nACGT\n"       # the space ends the token: its last byte '9' goes
                       b">EDGE_4\tx,y;\nACG\n"                               # a TAB does not end it
                       b">';\nAC\n"                                          # the empty name, primed
                       b">'':z;\nGT\n"                                       # V = '' : primed, the name one '
                       b">ab\n\n>a;b c\nTT\n>xy:,;\n>x,\nA\n>qr \nC\n>n\x0bm\x0c;\nG\n")
    cases["empty_sequences"] = b">E_1;\n>E_1';\n>E_2';\n\n>E_2;\n\n\n>E_3;\nAC\n\n>E_4;\n"
    cases["crlf_small"] = b">E_1:E_2';\r\nACGTAC\r\nGT\r\n>E_1':E_2;\r\nACGT\r\n>E_2;\r\n\r\n>E_3 x\r\nAC\r\n"
    cases["forward_other_bytes"] = b">E_1;\nacgtnNRYKM*-.\n>E_2;\nACGU\nacgu\n"
    cases["last_line_crlf"] = b">E_1';\nACGT\nAC\r\n>E_2;\nAC\r\n"
    cases["names_that_differ_by_prime_only"] = b">E_5':E_5;\nAACC\n>E_5;\nGGTT\n>E_5'';\nAC\n>E_5'';\nTT\n"
    return cases


def tile_sweep_texts(rng):
    """texts that put a header's '>', a record's last base and its LF, and the middle of a primed record on each of the offsets
    4090 .. 4100 (the index and the check kernels look at tiles of 4096 bytes)"""
    texts = []
    head = b">E_1;\n"
    for at in range(4088, 4103):
        first = head + dna(rng, at - len(head) - 1) + b"\n"                 # one line: its LF at at - 1, the next '>' at `at`
        assert len(first) == at
        texts.append(first + fold(b"E_2':E_1;", dna(rng, 150 + at % 16), 60) + fold(b"E_1':x;", dna(rng, 20), 60) + fold(b"E_3;", dna(rng, 9, b"acgtN"), 60))
    for at in range(4090, 4101):
        before = fold(b"E_9:E_8';", dna(rng, 3700 + at % 7, b"ACGTacgtn"), 60)
        assert len(before) < at - 100
        texts.append(before + fold(b"P_1';", dna(rng, 2 * (at - len(before)) + at % 16, b"ACGTacgt"), 70) + fold(b"P_1;", b"AC", 60))
    return texts


def residue_text(rng):
    """sixteen and more kept records whose output starts cover every residue mod 16 (names of growing length, sequences of growing
    length, both strands)"""
    out = []
    for i in range(40):
        out.append(fold(b"R" * (1 + i % 5) + b"_%d" % i + (b"';" if i % 2 else b";"), dna(rng, i * 6 % 37), 16))
    return b"".join(out)


def fault_cases():
    """{case: (text, code, 1-based line)}: one hand-made input per error"""
    good = b">E_1;\nACGT\nAC\n>E_1';\nGTAC\nGT\n"
    return {
        "plus_line": (good + b">E_2;\nAC\n+\nII\n", EPLUS, 9),
        "at_line": (b">E_1;\nACGT\n@E_2\nACGT\n", EPLUS, 3),
        "high_byte_in_header": (good + b">E_\xc3\xa9;\nAC\n", EHIGH, 7),
        "cr_inside_header": (b">E_1;\nAC\n>E_2\rx;\nAC\n", ECR, 3),
        "cr_cr_lf_header": (b">E_1;\r\r\nAC\n", ECR, 1),
        "no_final_lf": (good + b">E_2;\nACG", ENOLF, 8),
        "no_final_lf_header": (good + b">E_2;", ENOLF, 7),
        "empty_file": (b"", EEMPTY, 1),
        "empty_v": (good + b">:E_1;\nAC\n", ENONAME, 7),
        "one_byte_token": (b">E_1;\nAC\n>; x\nAC\n", ENONAME, 3),
        "primed_with_n": (good + b">E_2';\nACGT\nACNT\n", EBASE, 9),
        "primed_duplicate_with_n": (good + b">E_1';\nAC\nAn\n", EBASE, 9),
        "ragged": (b">E_1;\nACGT\nAC\nACGT\n", pc.ERAGGED, 4),
        "text_before": (b"AC\n" + good, pc.ETEXT, 1),
        "index_name": (good + b">\tx;\nAC\n", pc.ENAME, 7),
        "space_in_sequence": (good + b">E_2;\nA C\n", pc.EBYTE, 8),
        "two_faults": (good + b">E_2';\nACNT\n>E_3;\n+\n", EBASE, 8),
        "two_faults_one_line": (b">E_1;\nAC\n>\xff\r';\nAC\n", EHIGH, 3),
        "index_fault_behind_ours": (b">E_1';\nANGT\n>E_2;\nACGT\nAC\nACGT\n", EBASE, 2),
        "our_fault_behind_the_index": (b">E_1;\nACGT\nAC\nACGT\n>E_2';\nN\n", pc.ERAGGED, 4),
    }


def hand_checks():
    assert derive_name(b">EDGE_3_length_4_cov_9 extra:words;") == (b"EDGE_3_length_4_cov_", False)
    assert derive_name(b">EDGE_4\tx,y;") == (b"EDGE_4\tx", False)
    assert derive_name(b">';") == (b"", True) and derive_name(b">;") == (None, False) and derive_name(b">") == (None, False)
    assert derive_name(b">E_1':E_2;") == (b"E_1", True) and derive_name(b">E_1:") == (b"E_1", False)
    assert split_fastg(b">E_1:E_2';\nacgt\nNN\n>E_1';\nACGG\n>E_2';\nAACg\n>E_2;\nTT\n") == b">E_1\nacgtNN\n>E_2\nCGTT\n"
    assert split_fastg(b">E_1';\r\nAC\r\nG\r\n>E_2;\r\n") == b">E_1\nCGT\n>E_2\n\n"
    assert output_fai(b">E_1:E_2';\nacgt\nNN\n>E_2;\n") == b"E_1\t6\t5\t6\t7\nE_2\t0\t17\t0\t0\n"
    assert graph_fai(b">E_1:E_2';\nacgt\nNN\n>E_2;\n>E_1:E_2';\nAC\n") == (b"E_1:E_2';\t6\t11\t4\t5\nE_2;\t0\t25\t0\t0\n", [b"E_1:E_2';"])
    for name, (text, code, line) in fault_cases().items():
        assert verdict(text) == (code, line), (name, verdict(text), code, line)
    for name, text in golden_inputs().items():
        assert verdict(text) == (0, 0), (name, verdict(text))
    rng = np.random.default_rng(5)
    for t in tile_sweep_texts(rng) + [residue_text(rng)]:
        assert verdict(t) == (0, 0), verdict(t)


if __name__ == "__main__":
    hand_checks()
    print("split_fastg_cases: the restatement agrees with the hand-written files")
