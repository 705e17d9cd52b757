"""The record rules of palace_amd/csrc/bam_record.hpp -- the one text the host loader and the kernels of csrc/bam.hip are both compiled
from -- through the loader (`hostdump bam`), without a GPU.  The records are those of tests/test_gpu_bam_columns.py and
tests/test_gpu_bam_walk.py (builders imported, record lists restated: there they are locals of GPU tests); the expectations are the
hand values those tests state, expected_sa of tests/test_host_parsers.py with glibc's own atoi for the numbers, and serial_segments of
tests/test_gpu_bam_walk.py for the match segments.  Every file is also read by the ASan + UBSan build of hostdump (a stand-alone
CPU program), which must stay silent and print the same."""
import ctypes
import os
import struct
import subprocess

import pytest

from tests import test_host_parsers as parsers
from tests.test_gpu_bam_columns import N_REF, SA_OK, SA_TEXTS, TARGETS, aux_t, c_name, host_rows
from tests.test_gpu_bam_columns import random_records  # noqa: F401  (the fixture: 2 000 random records and hostdump's rows of them)
from tests.test_gpu_bam_walk import cg_record, serial_segments, serial_walk
from tests.test_host_bam_spec import HOST, HOSTDUMP, HOSTDUMP_ASAN, aux_A, aux_B, aux_C, aux_f, aux_i, aux_Z, cigar_words, header, record

NAMES = [n for n, _ in TARGETS]

_libc_atoi = ctypes.CDLL(None).atoi
_libc_atoi.restype = ctypes.c_int
_libc_atoi.argtypes = [ctypes.c_char_p]


def glibc_atoi(s):
    return _libc_atoi(s.encode("latin-1"))


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "hostdump"), os.path.join("..", "bin", "hostdump_asan")],
                   check=True, stdout=subprocess.DEVNULL)


def dump(tool, path):
    """the tool's output lines for `bam <path> 3 mseg`; nothing from a sanitizer on stderr"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([tool, "bam", path, "3", "mseg"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)
    assert b"AddressSanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr.decode()[:2000]
    assert p.returncode == 0, p.stderr
    lines = p.stdout.decode("latin-1").split("\n")
    assert lines[-1] == ""
    return lines[:-1]


def loaded(path, recs, targets=TARGETS, want=None):
    """-> (rows as host_rows gives them, match segments) of the loader, equal under the sanitizers"""
    if want is None:
        want = host_rows(path, targets, recs)                                      # (writes the BAM)
    lines = dump(HOSTDUMP, path)
    assert dump(HOSTDUMP_ASAN, path) == lines
    n = len(targets) + len(recs)
    assert [l.split("\t")[1:] for l in lines[len(targets):n]] == want and len(want) == len(recs)
    segs = [l.split("\t") for l in lines[n:]]
    assert all(s[0] == "MS" and len(s) == 4 for s in segs)
    return want, [tuple(int(x) for x in s[1:]) for s in segs]


def test_nm_and_aux_scan(tmp_path):
    recs = [record(f"nm_{ty}", 0, 0, 10, 60, "50M", aux=aux_t("NM", ty, v))
            for ty, v in (("c", -5), ("C", 200), ("s", -300), ("S", 60000), ("i", -70000), ("I", 4000000000), ("I", 7))]
    recs += [record("nm_A_first", 0, 0, 10, 60, "50M", aux=aux_A("NM", "7") + aux_i("NM", 9)),            # the first NM decides: 0
             record("nm_f_first", 0, 0, 10, 60, "50M", aux=aux_f("NM", 3.5) + aux_C("NM", 9)),
             record("nm_Z_first", 0, 0, 10, 60, "50M", aux=aux_Z("NM", "12") + aux_C("NM", 9)),
             record("nm_twice", 0, 0, 10, 60, "50M", aux=aux_C("NM", 3) + aux_C("NM", 9)),
             record("nm_none", 0, 0, 10, 60, "50M", aux=aux_Z("XX", "y")),
             record("sa_A_first", 0, 0, 10, 60, "50M", aux=aux_A("SA", "x") + aux_Z("SA", SA_OK) + aux_C("NM", 4)),     # an SA:A does not end the search
             record("sa_twice", 0, 0, 10, 60, "50M", aux=aux_Z("SA", SA_OK) + aux_Z("SA", "b,1,+,10M,1,1;") + aux_C("NM", 4)),
             record("unknown_first", 0, 0, 10, 60, "50M", aux=b"XQ?abcd" + aux_C("NM", 4) + aux_Z("SA", SA_OK)),       # the scan stops: nm 0, no items
             record("open_z", 0, 0, 10, 60, "50M", aux=aux_C("NM", 4) + b"SAZ" + b"c10,15,-,30S70M,40,2"),            # a string past the record
             record("big_b", 0, 0, 10, 60, "50M", aux=b"ZBBi" + struct.pack("<i", 0x7fffffff) + aux_C("NM", 3)),
             record("both_found", 0, 0, 10, 60, "50M", aux=aux_C("NM", 1) + aux_Z("SA", SA_OK) + b"XQ?" + aux_C("NM", 9)),
             record("arrays", 0, 0, 10, 60, "50M", aux=aux_B("ZB", "c", [-1, 2]) + aux_B("ZC", "S", [1, 65535]) + aux_B("ZE", "I", []) + aux_t("NM", "s", 11))]
    want, segs = loaded(str(tmp_path / "t.bam"), recs)
    assert [w[6] for w in want[:7]] == ["-5", "200", "-300", "60000", "-70000", str(4000000000 - (1 << 32)), "7"]
    assert [w[6] for w in want[7:12]] == ["0", "0", "0", "3", "0"]
    assert want[12][6] == "4" and want[12][11:] == ["SA:2,15,1,40,2,30,0,100"] and len(want[13]) == 12
    assert want[14][6] == "0" and len(want[14]) == 11 and want[15][6] == "4" and len(want[15]) == 11
    assert want[16][6] == "0" and want[17][6] == "1" and len(want[17]) == 12 and want[18][6] == "11"
    assert segs == [(0, 10, 50)] * len(recs)


def test_cigars_names_and_tids(tmp_path):
    no_nul = bytearray(record("abcdef", 0, 1, 5, 60, "10M"))
    no_nul[36 + 6] = ord("g")                                                          # no NUL inside l_read_name: l_read_name - 1 bytes
    early = bytearray(record("abXcd", 0, 1, 5, 60, "10M"))
    early[36 + 2] = 0
    recs = [record("nocig", 0, 1, 30, 60, "", l_seq=12),
            record("nocig_unmapped", 4, -1, -1, 0, ""),
            record("zero_ops", 0, 1, 20, 60, "0M5M0D0=3X0N"),
            record("zero_lead_s", 0, 1, 20, 60, "0S10M4S"),
            record("zero_trail_s", 0, 1, 20, 60, "4S10M0S"),
            record("only_zero", 0, 1, 20, 60, "0M0S"),
            record("s_alone", 0, 1, 20, 60, "100S"),
            record("s_both", 0, 1, 20, 60, "5S10M7S"),
            record("h_then_s", 0, 1, 20, 60, "5H5S10M3S2H"),
            record("mix", 0, 2, 1000, 60, "5S10M2D3I7M100N4=1X2P6M5H"),
            record("op_b", 0, 1, 20, 60, [(4 << 4) | 9, (10 << 4) | 0, (3 << 4) | 15], l_seq=10),
            bytes(no_nul), bytes(early),
            record("nuls", 99, 1, 0, 0, "100M", mtid=1, mpos=300, name_extra_nul=3),
            record("tid-1_sa", 0, -1, 10, 60, "10M", aux=aux_Z("SA", SA_OK)),
            record("tid_n_ref_sa", 0, N_REF, 10, 60, "10M", aux=aux_Z("SA", SA_OK) + aux_C("NM", 2)),
            record("tid_big_sa", 0, 1 << 20, 10, 60, "10M", aux=aux_Z("SA", SA_OK)),
            record("last_tid_sa", 0x10, N_REF - 1, 10, 3, "10M", mtid=N_REF - 1, mpos=-1, aux=aux_Z("SA", SA_OK))]
    want, _ = loaded(str(tmp_path / "t.bam"), recs)
    by = dict(zip((c_name(r).decode() for r in recs), want))
    assert by["nocig"][7:11] == ["0", "0", "-1", "0"] and by["only_zero"][9:11] == ["0", "0"]
    assert by["s_alone"][9:11] == ["100", "0"] and by["s_both"][9:11] == ["5", "7"] and by["h_then_s"][9:11] == ["0", "0"]
    assert by["zero_lead_s"][9:11] == ["0", "4"] and by["zero_trail_s"][9:11] == ["4", "0"]
    assert "abcdef" in by and "ab" in by                                # (seven bytes without a NUL: the first six; cut at the early NUL)
    assert len(by["tid-1_sa"]) == len(by["tid_n_ref_sa"]) == len(by["tid_big_sa"]) == 11 and len(by["last_tid_sa"]) == 12
    assert by["mix"][7:11] == ["130", "36", "5", "0"] and by["zero_ops"][7:9] == ["8", "8"] and by["op_b"][7:11] == ["10", "10", "0", "0"]


def test_sa_texts(tmp_path, monkeypatch):
    """every text on a record of contig c1 (so that `c1` is the record's own contig), and the name cases on the two `dup` contigs;
    the numbers are what glibc's atoi makes of the trimmed fields"""
    monkeypatch.setattr(parsers, "atoi", glibc_atoi)
    own = [1] * len(SA_TEXTS) + [4, 6, 0]
    texts = SA_TEXTS + ["dup,5,+,10M,60,0;c1,6,-,10M,60,0;"] * 2 + ["c,5,+,10M,60,0;c1,6,-,10M,60,0;c10,7,+,,1,1"]
    recs = [record(f"sa{k}", 0, tid, 10, 60, "40M60S", aux=aux_C("NM", 1) + aux_Z("SA", t)) for k, (tid, t) in enumerate(zip(own, texts))]
    want, _ = loaded(str(tmp_path / "t.bam"), recs)
    for t, tid, w in zip(texts, own, want):
        assert w[11:] == ["SA:" + ",".join(str(x) for x in item) for item in parsers.expected_sa(t, NAMES, tid)], t
    items = {t: w[11:] for t, w in zip(SA_TEXTS, want)}
    # the definition itself, on what can be said by hand
    assert items["zzz,5,+,60S40M,60,0"] == ["SA:-1,5,0,60,0,60,0,100"] and items["c1,5,+"] == [] and items[",,,,,"] == []
    assert items["c1,x,+,60S40M,60,0"] == ["SA:-1,0,0,60,0,60,0,100"] and items["c10,5,+,60S40M,60"] == [] and items["c10,5,+,60S40M,60,"] == []
    assert items["c10,5,+,60S40M,60,,"] == ["SA:2,5,0,60,0,60,0,100"]
    assert items[SA_TEXTS[5]] == ["SA:2,5,1,60,0,60,0,100", "SA:5,7,1,30,1,0,60,100"]
    assert items["c10,2147483648,+,10M,60,0"][0].split(",")[1] == "-2147483648"
    assert items["c10,99999999999999999999,+,10M,60,0"][0].split(",")[1] == "-1"
    assert items["c10,-99999999999999999999,+,10M,60,0"][0].split(",")[1] == "0"
    assert items["c10,5,+,,60,0"] == ["SA:2,5,0,60,0,-1,0,0"] and items["c10,5,+,10Q40M50S,60,0"] == ["SA:2,5,0,60,0,0,50,90"]
    assert items["dup,5,+,10M,60,0"] == ["SA:6,5,0,60,0,0,0,10"] and items["c1,5,+,10M,60,0"] == ["SA:-1,5,0,60,0,0,0,10"]
    assert [i.split(",")[0] for i in (items["c,5,+,10M,60,0"] + items["c1a,5,+,10M,60,0"] + items["c1b,5,+,10M,60,0"])] == ["SA:0", "SA:3", "SA:-1"]
    assert len(items[SA_TEXTS[-1]]) == 40
    assert [i.split(",")[0] for i in want[-3][11:]] == ["SA:-1", "SA:1"] and [i.split(",")[0] for i in want[-2][11:]] == ["SA:-1", "SA:1"]
    assert [i.split(",")[0] for i in want[-1][11:]] == ["SA:-1", "SA:1", "SA:2"]


def test_match_segments(tmp_path):
    """the records of test_segment_rules of tests/test_gpu_bam_walk.py and its CG:B,I record of 70 000 ops, on three contigs"""
    targets = [("a", 5000), ("b", 5000), ("c", 200000)]
    ops40 = cigar_words("1M1D" * 40)
    cg = lambda name, aux, pos=7: record(name, 0, 2, pos, 30, [(40 << 4) | 4, (80 << 4) | 3], l_seq=40, aux=aux)
    recs = [record("m", 0, 0, 100, 60, "20S80M"),
            record("rev", 0x10, 1, 5, 60, "50M")]
    recs += [record(f"f{f:x}", f, 0, 10, 60, "10M") for f in (0x4, 0x100, 0x200, 0x400, 0x800)]         # only 0x800 counts
    recs += [record("tid-1", 0, -1, 10, 60, "10M"), record("tid3", 0, 3, 10, 60, "10M"), record("tid9", 0, 9, 10, 60, "10M"),
             record("pos-1", 0, 1, -1, 60, "10M"),
             record("zero", 0, 1, 20, 60, "0M5M0D0=3X0N"),
             record("mix", 0, 2, 1000, 60, "5S10M2D3I7M100N4=1X2P6M5H"),
             record("nocig", 0, 1, 30, 60, "", l_seq=12),
             cg("cg", aux_i("NM", 1) + aux_B("CG", "I", ops40)),
             cg("cg_i", aux_B("CG", "i", ops40)),                                                         # subtype i is taken too
             cg("cg_wrong_type", aux_B("CG", "S", [w & 0xffff for w in ops40])),                          # ignored: the placeholder stays
             cg("cg_z", aux_Z("CG", "80M")),
             cg("cg_short", aux_B("CG", "I", [(5 << 4) | 0])),                                            # count < n_cigar_op: ignored
             cg("cg_twice", aux_B("CG", "S", [1, 2]) + aux_B("CG", "I", ops40)),                          # the first CG tag decides
             cg("cg_twice2", aux_B("CG", "I", ops40) + aux_B("CG", "I", cigar_words("40M"))),
             cg("cg_behind_unknown", b"XQ?" + b"abcd" + aux_B("CG", "I", ops40)),                        # unknown type: the scan stops
             cg("cg_behind_open_z", b"XZZ" + b"no end"),                                                 # a string that runs past the record
             cg("cg_negpos", aux_B("CG", "I", ops40), pos=-1),
             record("fake", 0, 2, 9, 30, [(50 << 4) | 4, (60 << 4) | 3], l_seq=50),
             record("last", 0, 0, 4000, 60, "30=5X15M", aux=aux_A("XA", "q")),
             cg_record()]
    stream = header(targets) + b"".join(recs)
    starts, stop = serial_walk(stream, len(header(targets)))
    assert len(starts) == len(recs) and stop == len(stream)
    exp = serial_segments(stream, starts, len(targets))
    # the restatement itself, on what can be said by hand
    assert exp[:3] == [(0, 100, 80), (1, 5, 50), (0, 10, 10)]
    assert (1, 20, 5) in exp and (1, 25, 3) in exp and (2, 1000, 10) in exp and (2, 1012, 7) in exp and (2, 1119, 4) in exp and (2, 1124, 6) in exp
    assert exp[-35000:] == [(2, 7 + 2 * k, 1) for k in range(35000)]                                   # the long record
    assert sum(1 for s in exp[:-35000] if s[0] == 2 and s[2] == 1 and 7 <= s[1] < 7 + 80) == 40 * 3    # cg, cg_i, cg_twice2: the tag is taken
    want, segs = loaded(str(tmp_path / "t.bam"), recs, targets)
    assert segs == exp
    assert want[-1][6:11] == ["1", "70000", "35000", "0", "0"]


def test_random_records_under_sanitizers(random_records, tmp_path):
    """the 2 000 random records of tests/test_gpu_bam_columns.py: the sanitized loader prints what the plain one printed, and the match
    segments are those of the serial restatement"""
    recs, want = random_records
    path = str(tmp_path / "r.bam")
    assert host_rows(path, TARGETS, recs) == want
    _, segs = loaded(path, recs, want=want)
    stream = header(TARGETS) + b"".join(recs)
    starts, _ = serial_walk(stream, len(header(TARGETS)))
    assert len(starts) == len(recs) and segs == serial_segments(stream, starts, N_REF)
