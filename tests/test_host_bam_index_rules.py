"""sort_key, bai_span and reg2bin of palace_amd/csrc/bam_record.hpp -- the one statement the kernels of bam_sort.hip / bam_index.hip
and the host share -- through the stand-alone `bam_index_selftest`, as built and under AddressSanitizer + UBSan, against the Python
restatement of tests/bam_sort_cases.py; the bins also against the reg2bins of tests/tabix_reader.py (a record's bin must be among the
bins a reader looks through for the record's own interval)."""
import os
import random
import subprocess

import pytest

from tests import bam_sort_cases as bc
from tests.tabix_reader import reg2bins
from tests.test_host_bam_spec import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
TOOLS = [os.path.join(ROOT, "palace_amd", "bin", n) for n in ("bam_index_selftest", "bam_index_selftest_asan")]
N_REF = 7


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", os.path.basename(t)) for t in TOOLS], check=True, stdout=subprocess.DEVNULL)


def expected_line(rec, n_ref):
    beg, end = bc.span(rec)
    key = str(bc.sort_key(rec, n_ref)) if bc.key_ok(rec, n_ref) else "bad"
    return f"{key}\t{beg}\t{end}\t{bc.reg2bin(beg, end) if bc.indexable(rec) else -1}"


def check(tmp_path, recs, n_ref=N_REF):
    path = tmp_path / "records.bin"
    path.write_bytes(b"".join(recs))
    want = [expected_line(r, n_ref) for r in recs]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    for tool in TOOLS:
        p = subprocess.run([tool, str(path), str(n_ref)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
        assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[:2000]
        assert p.returncode == 0, p.stderr.decode()
        assert p.stdout.decode().splitlines() == want
    for r in recs:                                                           # the restatement against the reader's side of the scheme
        if bc.indexable(r):
            beg, end = bc.span(r)
            assert bc.reg2bin(beg, end) in reg2bins(beg, end)
    return want


def test_hand_cases(tmp_path):
    recs = [
        record("pos_minus_1", 0, 2, -1, 0, "10M"),                           # sorts in front of pos 0; a .bai cannot hold it
        record("unplaced_with_pos", 4, -1, 777, 0, "", l_seq=5),             # refID -1 with a position: keyed behind every contig
        record("reverse", 16, 1, 100, 60, "50M"),
        record("forward", 0, 1, 100, 60, "50M"),
        record("zero_m", 0, 1, 200, 60, "0M", l_seq=4),                      # ops, but no reference bases: one base
        record("only_s_i", 0, 1, 300, 60, "5S7I"),
        record("unmapped_with_cigar", 4, 1, 400, 0, "30M"),                  # flag 0x4: one base whatever the CIGAR says
        record("no_ops", 0, 3, 16383, 0, "", l_seq=9),
        bc.cg_record("cg", 0, 2, 7, "10S" + "1M1D" * 40 + "50M5S"),
        record("fake_placeholder", 0, 2, 9, 30, [(50 << 4) | 4, (60 << 4) | 3], l_seq=50),
        record("bad_tid", 0, N_REF, 5, 0, "5M"),
        record("bad_tid_low", 0, -2, 5, 0, "5M"),
        record("bad_pos", 0, 0, -2, 0, "5M"),
        record("past_the_scheme", 0, 0, (1 << 29) - 3, 0, "4M"),             # end = 2^29 + 1
    ]
    for shift in (14, 17, 20, 23, 26, 29):                                   # spans that end exactly on a level's boundary, and one past it
        edge = 1 << shift
        recs += [record(f"on_{shift}", 0, 0, edge - 40, 0, "40M"), record(f"before_{shift}", 0, 0, edge - 41, 0, "40M")]
        if shift < 29:
            recs += [record(f"across_{shift}", 0, 0, edge - 39, 0, "40M"), record(f"at_{shift}", 0, 0, edge, 0, "1M")]
    want = check(tmp_path, recs)
    by_name = dict(zip((r[36:r.index(b"\0", 36)].decode() for r in recs), (w.split("\t") for w in want)))
    assert by_name["pos_minus_1"][3] == "-1" and by_name["past_the_scheme"][3] == "-1" and by_name["on_29"][3] == str(4681 + 32767)
    assert by_name["bad_tid"][0] == by_name["bad_tid_low"][0] == by_name["bad_pos"][0] == "bad"
    assert int(by_name["forward"][0]) + 1 == int(by_name["reverse"][0])
    assert int(by_name["unplaced_with_pos"][0]) >> 33 == N_REF
    assert [by_name[k][1:3] for k in ("zero_m", "only_s_i", "unmapped_with_cigar")] == [["200", "201"], ["300", "301"], ["400", "401"]]
    assert by_name["cg"][2] == str(7 + 80 + 50) and by_name["fake_placeholder"][2] == str(9 + 60)
    assert by_name["on_14"][3] == "4681" and by_name["across_14"][3] == "585" and by_name["across_26"][3] == "0"


def test_random_records(tmp_path):
    rng = random.Random(20250)
    targets = [("a", 1 << 29), ("b", 5000), ("c", 300000), ("d", 70000), ("e", 1 << 20), ("f", 1 << 27), ("g", 40)]
    recs = bc.random_records(rng, 2000, targets, unplaced=0.1)
    check(tmp_path, recs, n_ref=len(targets))
