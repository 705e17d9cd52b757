"""The rules of faidx on a CPU.  Parity with `samtools faidx` is UNPINNED -- samtools, htslib, pyfaidx, pysam and
Biopython are all absent -- so the restatement of tests/faidx_cases.py IS the definition, and this file pins it: a catalogue whose
expected stdout, stderr and exit status were typed by hand from the rules, not copied from any program's output.  Beside it,
csrc/faidx_region.hpp -- the grammar the kernel of csrc/faidx.hip compiles -- driven by the stand-alone `faidx_region_selftest`
(its own main, every region in an allocation of exactly its length), as built and under ASan + UBSan with nothing preloaded."""
import os
import subprocess

import pytest

from tests import faidx_cases as fx
from tests.path_fasta_cases import fasta_index, first_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
NAMES = ("faidx_region_selftest", "faidx_region_selftest_asan")
TOOLS = [os.path.join(BIN, t) for t in NAMES]

FAILED = b"[faidx] Failed to fetch sequence in "
ZERO = b"[faidx] Zero length sequence: "

# (case, options of fx.fetch, regions, stdout, stderr, exit status) over fx.CATALOGUE_FASTA:
#   chr1   ACGTACGTAC GTACGTACGT ACGTA (25)     a:b  AAAACCCCGG (10)     a:b:2-3  TTTT     chr1 again  GGGG (never found)
#   ambi   RYKMBVDHSWN acgtn* (17)              empty (0)                p|q|r    ACGTACGTACGT (12)
CATALOGUE = [
    ("whole_record", {}, [b"chr1"], b">chr1\nACGTACGTACGTACGTACGTACGTA\n", b"", 0),
    ("whole_record_lines_of_10", {"n": 10}, [b"chr1"], b">chr1\nACGTACGTAC\nGTACGTACGT\nACGTA\n", b"", 0),
    ("b_to_e", {}, [b"chr1:3-12"], b">chr1:3-12\nGTACGTACGT\n", b"", 0),
    ("b_to_e_across_source_lines", {"n": 4}, [b"chr1:9-14"], b">chr1:9-14\nACGT\nAC\n", b"", 0),
    ("up_to_e", {}, [b"chr1:-4"], b">chr1:-4\nACGT\n", b"", 0),
    ("from_b", {}, [b"chr1:21-"], b">chr1:21-\nACGTA\n", b"", 0),
    ("b_alone_is_from_b", {}, [b"chr1:22"], b">chr1:22\nCGTA\n", b"", 0),
    ("commas", {}, [b"chr1:1,0-1,2"], b">chr1:1,0-1,2\nCGT\n", b"", 0),
    ("b_zero_counts_as_one", {}, [b"chr1:0-3"], b">chr1:0-3\nACG\n", b"", 0),
    ("e_clipped", {}, [b"chr1:20-99"], b">chr1:20-99\nTACGTA\n", b"", 0),
    ("b_beyond_the_end", {}, [b"chr1:26-30"], b">chr1:26-30\n", ZERO + b"chr1:26-30\n", 0),
    ("e_below_b", {}, [b"chr1:5-4"], b"", FAILED + b"chr1:5-4\n", 1),
    ("colon_name_whole_string_is_a_record", {}, [b"a:b:2-3"], b">a:b:2-3\nTTTT\n", b"", 0),
    ("colon_name_only_the_cut_form", {}, [b"a:b:2-4"], b">a:b:2-4\nAAA\n", b"", 0),
    ("colon_name_whole", {}, [b"a:b"], b">a:b\nAAAACCCCGG\n", b"", 0),
    ("duplicate_name_first_is_found", {}, [b"chr1:1-4"], b">chr1:1-4\nACGT\n", b"", 0),
    ("pipes_in_a_name", {}, [b"p|q|r"], b">p|q|r\nACGTACGTACGT\n", b"", 0),
    ("reverse_mark_rc", {"reverse": True}, [b"ambi"], b">ambi/rc\n*nacgtNWSDHBVKMRY\n", b"", 0),
    ("reverse_mark_sign", {"reverse": True, "mark": "sign"}, [b"chr1:1-5"], b">chr1:1-5(-)\nTACGT\n", b"", 0),
    ("reverse_mark_no", {"reverse": True, "mark": "no"}, [b"chr1:22-25"], b">chr1:22-25\nTACG\n", b"", 0),
    ("forward_mark_sign", {"mark": "sign"}, [b"chr1:1-2"], b">chr1:1-2(+)\nAC\n", b"", 0),
    ("forward_mark_no", {"mark": "no"}, [b"chr1:1-2"], b">chr1:1-2\nAC\n", b"", 0),
    ("lines_of_one", {"n": 1}, [b"a:b:3-6"], b">a:b:3-6\nA\nA\nC\nC\n", b"", 0),
    ("body_is_a_multiple_of_n", {"n": 5}, [b"a:b"], b">a:b\nAAAAC\nCCCGG\n", b"", 0),
    ("empty_record", {}, [b"empty"], b">empty\n", ZERO + b"empty\n", 0),
    ("unknown_name", {}, [b"chr2"], b"", FAILED + b"chr2\n", 1),
    ("braces_are_not_special", {}, [b"{chr1}:1-5"], b"", FAILED + b"{chr1}:1-5\n", 1),
    ("first_failure_and_nothing_else", {}, [b"chr1:1-2", b"chr1:x", b"chr2"], b"", FAILED + b"chr1:x\n", 1),
    ("keep_going", {"keep_going": True}, [b"chr1:1-2", b"chr1:x", b"chr1:99", b"chr2", b"a:b:9-"],
     b">chr1:1-2\nAC\n>chr1:99\n>a:b:9-\nGG\n", FAILED + b"chr1:x\n" + ZERO + b"chr1:99\n" + FAILED + b"chr2\n", 0),
]


def test_the_catalogue_has_the_cases_the_rules_name():
    assert len(CATALOGUE) >= 12 and len({c[0] for c in CATALOGUE}) == len(CATALOGUE)


@pytest.mark.parametrize("case", CATALOGUE, ids=[c[0] for c in CATALOGUE])
def test_restatement_against_the_hand_typed_catalogue(case):
    _, options, regions, stdout, stderr, status = case
    assert fx.fetch(fx.CATALOGUE_FASTA, regions, **options) == (stdout, stderr, status)


# (region, rec, beg, len) typed by hand: records 0 chr1 (25), 1 a:b (10), 2 a:b:2-3 (4), 3 chr1 again, 4 ambi (17), 5 empty (0), 6 p|q|r (12)
RESOLVED_BY_HAND = [
    (b"chr1", 0, 0, 25), (b"chr1:3-12", 0, 2, 10), (b"chr1:-4", 0, 0, 4), (b"chr1:21-", 0, 20, 5), (b"chr1:0", 0, 0, 25), (b"chr1:25-25", 0, 24, 1),
    (b"chr1:26", 0, 25, 0), (b"chr1:1000000-", 0, 25, 0), (b"chr1:5-4", -1, 0, 0), (b"chr1:0-0", -1, 0, 0), (b"chr1:-0", -1, 0, 0), (b"a:b:2-3", 2, 0, 4),
    (b"a:b:2-4", 1, 1, 3), (b"a", -1, 0, 0), (b"a:", -1, 0, 0), (b"chr1:", -1, 0, 0), (b"chr1:-", -1, 0, 0), (b"chr1:,", -1, 0, 0), (b"chr1:,1,", 0, 0, 25),
    (b"chr1:3-12x", -1, 0, 0), (b"chr1:3--4", -1, 0, 0), (b"chr1: 3", -1, 0, 0), (b"chr1 ", -1, 0, 0), (b"CHR1", -1, 0, 0), (b"empty", 5, 0, 0),
    (b"empty:1-5", 5, 0, 0), (b"p|q|r:2-3", 6, 1, 2), (b"chr1:123456789012345678", 0, 25, 0), (b"chr1:1-123456789012345678", 0, 0, 25),
    (b"chr1:1234567890123456789", -1, 0, 0), (b"chr1:1-1234567890123456789", -1, 0, 0), (b"chr1:0000000000000000001", -1, 0, 0),
    (b"chr1:000000000000000001-000000000000000002", 0, 0, 2), (b":", -1, 0, 0), (b"", -1, 0, 0), (b"chr1:chr1:2-3", -1, 0, 0),
]


def model_resolved(regions):
    recs, code, _ = fasta_index(fx.CATALOGUE_FASTA)
    assert code == 0
    first_of = first_records(recs)
    return [fx.resolve(r, recs, first_of) for r in regions]


def test_restatement_resolves_as_typed_by_hand():
    assert set(r for r, *_ in RESOLVED_BY_HAND) - {b""} <= set(fx.GRAMMAR_REGIONS)
    assert model_resolved([r for r, *_ in RESOLVED_BY_HAND]) == [tuple(w) for _, *w in RESOLVED_BY_HAND]


@pytest.fixture(scope="module")
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in NAMES], check=True, stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_grammar_header_against_the_restatement(built, tool, tmp_path):
    recs, _, _ = fasta_index(fx.CATALOGUE_FASTA)
    (tmp_path / "records.txt").write_bytes(b"".join(b"%s\t%d\n" % (r["name"], r["length"]) for r in recs))
    regions = fx.GRAMMAR_REGIONS + [b"", b"chr1"]                                # an empty region in the middle: a line of its own
    (tmp_path / "regions.txt").write_bytes(b"\n".join(regions) + b"\n")
    p = subprocess.run([tool, str(tmp_path / "records.txt"), str(tmp_path / "regions.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]               # (a sanitizer report goes to stderr and ends the run)
    got = [tuple(int(x) for x in line.split()) for line in p.stdout.split(b"\n")[:-1]]
    want = model_resolved(regions)
    assert len(got) == len(want)
    for region, g, w in zip(regions, got, want):
        assert g == w, (region, g, w)
    assert sum(w[0] < 0 for w in want) > 20 and sum(w[0] >= 0 and w[2] > 0 for w in want) > 15 and sum(w[0] >= 0 and w[2] == 0 for w in want) > 4
