"""palace_bam_columns, palace_bam_sa_items, palace_bam_name_keys and palace_bam_names_differ (palace_amd/csrc/bam.hip) through the C
ABI.  The expectation is the host loader's own decode (BamLoad::decode_range, palace_amd/host/bam.cpp), read through `hostdump bam`:
that loader is the definition.  The same records are written once as a BAM for hostdump and once as a raw stream for the device, which
runs walk -> columns -> SA items; every column, sa_off and every item field must be equal.  qkey, which hostdump does not print, is
checked against the statement of name_key below."""
import os
import struct
import subprocess

import numpy as np
import pytest

from palace_amd import capi, synth
from tests.test_gpu_bam_walk import cg_record
from tests.test_host_bam_spec import EOF_MEMBER, aux_A, aux_B, aux_C, aux_f, aux_i, aux_Z, bgzf_member, header, record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
HOSTDUMP = os.path.join(ROOT, "palace_amd", "bin", "hostdump")

# names that are prefixes of each other, and one name on two contigs (the last one is what a look-up finds)
TARGETS = [("c", 1000), ("c1", 2000), ("c10", 3000), ("c1a", 500), ("dup", 100), ("b", 700), ("dup", 900)]
N_REF = len(TARGETS)
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(HOSTDUMP):
        subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "hostdump")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="module")
def ctx():
    with capi.Ctx(0) as c:
        yield c


def name_key(name: bytes, seed: int) -> int:
    """name_key of palace_amd/host/bam.cpp"""
    h = 0xcbf29ce484222325 ^ ((seed * 0x9e3779b97f4a7c15) & M64)
    for ch in name:
        h = ((h ^ ch) * 0x100000001b3) & M64
    h ^= h >> 32
    h = (h * 0xd6e8feb86659fd93) & M64
    return h ^ (h >> 32)


def c_name(rec: bytes) -> bytes:
    """the C-string view of an encoded record's name"""
    l_name = rec[4 + 8]
    raw = rec[36:36 + l_name]
    z = raw.find(b"\0")
    return raw[:z] if z >= 0 else raw[:l_name - 1]


def host_rows(path, targets, recs):
    """what the host loader decodes: per record the list of its printed fields behind the name, SA items included"""
    stream = header(targets) + b"".join(recs)
    with open(path, "wb") as f:
        for a in range(0, len(stream), 60000):
            f.write(bgzf_member(stream[a:a + 60000], level=1))
        f.write(EOF_MEMBER)
    p = subprocess.run([HOSTDUMP, "bam", path, "3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.decode("latin-1").split("\n")[len(targets):]
    assert lines[-1] == ""
    return [l.split("\t")[1:] for l in lines[:-1]]


def device_rows(ctx, targets, recs, chunk=0, key_seed=1):
    stream = header(targets) + b"".join(recs)
    first = len(header(targets))
    starts, stop, _ = capi.bam_walk(ctx, stream, first, len(targets), chunk)
    cols, items = capi.bam_decode(ctx, stream, starts, [n.encode() for n, _ in targets], key_seed)
    assert cols["sa_off"][0] == 0 and cols["sa_off"][-1] == len(items) and np.all(np.diff(cols["sa_off"]) >= 0)
    rows = []
    for i in range(len(starts)):
        row = [str(int(cols[k][i])) for k in ("flag", "tid", "pos", "mapq", "mtid", "mpos", "nm", "ref_len", "read_len", "clip_s", "clip_e")]
        for s in items[cols["sa_off"][i]:cols["sa_off"][i + 1]]:
            row.append("SA:" + ",".join(str(int(s[k])) for k in ("tid2", "pos2", "rev2", "mapq2", "nm2", "clip_s2", "clip_e2", "len2")))
        rows.append(row)
    return rows, cols


def same(ctx, tmp_path, recs, targets=TARGETS, chunk=0):
    want = host_rows(str(tmp_path / "t.bam"), targets, recs)
    got, cols = device_rows(ctx, targets, recs, chunk)
    assert len(want) == len(recs) == len(got)
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == w, (i, c_name(recs[i]))
    assert cols["qkey"].tolist() == [name_key(c_name(r), 1) for r in recs]
    return want


def aux_t(tag, ty, v):
    return tag.encode() + ty.encode() + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I"}[ty], v)


SA_OK = "c10,15,-,30S70M,40,2;"


def test_nm_and_aux_scan(ctx, tmp_path):
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
    want = same(ctx, tmp_path, recs)
    assert [w[6] for w in want[:7]] == ["-5", "200", "-300", "60000", "-70000", str(4000000000 - (1 << 32)), "7"]
    assert [w[6] for w in want[7:12]] == ["0", "0", "0", "3", "0"]
    assert want[12][6] == "4" and want[12][11:] == ["SA:2,15,1,40,2,30,0,100"] and len(want[13]) == 12
    assert want[14][6] == "0" and len(want[14]) == 11 and want[15][6] == "4" and len(want[15]) == 11


def test_cigars_names_and_tids(ctx, tmp_path):
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
    want = same(ctx, tmp_path, recs)
    by = dict(zip((c_name(r).decode() for r in recs), want))
    assert by["nocig"][7:11] == ["0", "0", "-1", "0"] and by["only_zero"][9:11] == ["0", "0"]
    assert by["s_alone"][9:11] == ["100", "0"] and by["s_both"][9:11] == ["5", "7"] and by["h_then_s"][9:11] == ["0", "0"]
    assert by["zero_lead_s"][9:11] == ["0", "4"] and by["zero_trail_s"][9:11] == ["4", "0"]
    assert "abcdef" in by and "ab" in by                                # (seven bytes without a NUL: the first six; cut at the early NUL)
    assert len(by["tid-1_sa"]) == len(by["tid_n_ref_sa"]) == len(by["tid_big_sa"]) == 11 and len(by["last_tid_sa"]) == 12


SA_TEXTS = [
    "zzz,5,+,60S40M,60,0", "c1,5,+", ",,,,,", "c1,x,+,60S40M,60,0", "c1,5,+,60S40M,60",                  # the malformed ones of test_gpu_graph_fuzz.py
    " c10 ,\t5\t, - ,60S40M , 60 ,\t0 ;\tb\t, 7,-\t,\t40M60S, 30 , 1\t",                                  # blanks and tabs around every field
    "\vc10\f,5\r,+\n,10M,60,0",
    "c10,5,+,60S40M,60,0;;b,7,-,40M60S,30,1;", ";;", ";", ";c10,5,+,60S40M,60,0",
    "c10,5,+,60S40M,60", "c10,5,+,60S40M,60,", "c10,5,+,60S40M,60,,", "c10,5,+,60S40M,60,0,extra,fields",
    "c10,+7,+,10M,60,0", "c10,-3,+,10M,60,0", "c10,12x,+,10M,60,0", "c10,x,+,10M,60,0", "c10,2147483648,+,10M,60,0",
    "c10,99999999999999999999,+,10M,60,0", "c10,-99999999999999999999,+,10M,60,0", "c10,9223372036854775807,+,10M,60,0",
    "c10,-9223372036854775808,+,10M,60,0", "c10,4294967301,+,10M,+60,-0", "c10,- 3,+,10M,6 0,1 2", "c10,+,+,10M,-,+",
    "c10,5,+,10Q40M50S,60,0", "c10,5,+,5S3Z,60,0", "c10,5,+,S,60,0", "c10,5,+,M10,60,0", "c10,5,+,10,60,0", "c10,5,+,,60,0",
    "c10,5,+,0S10M0S,60,0", "c10,5,+,7S,60,0", "c10,5,+,3S10m4s,60,0", "c10,5,+,4S 10M,60,0",
    "c10,5,-,10M,60,0", "c10,5,--,10M,60,0", "c10,5,,10M,60,0", "c10,5, - ,10M,60,0",
    "c1,5,+,10M,60,0", "c,5,+,10M,60,0", "c10,5,+,10M,60,0", "c1a,5,+,10M,60,0", "c1b,5,+,10M,60,0", "c100,5,+,10M,60,0", "C1,5,+,10M,60,0",
    "dup,5,+,10M,60,0", "b,5,+,10M,60,0", " ,5,+,10M,60,0", "c10, ,+,10M,60,0", "c10,5,+,10M, , ",
    ";".join("%s,%d,%s,%dS%dM,60,%d" % (TARGETS[k % N_REF][0], k, "+-"[k % 2], k, 100 - k, k % 7) for k in range(40)) + ";",
]


def test_sa_texts(ctx, tmp_path):
    """every text on a record of contig c1 (so that `c1` is the record's own contig), and the name cases on the two `dup` contigs"""
    recs = [record(f"sa{k}", 0, 1, 10, 60, "40M60S", aux=aux_C("NM", 1) + aux_Z("SA", t)) for k, t in enumerate(SA_TEXTS)]
    recs += [record("on_dup_first", 0, 4, 10, 60, "40M", aux=aux_Z("SA", "dup,5,+,10M,60,0;c1,6,-,10M,60,0;")),
             record("on_dup_last", 0, 6, 10, 60, "40M", aux=aux_Z("SA", "dup,5,+,10M,60,0;c1,6,-,10M,60,0;")),
             record("on_c", 0, 0, 10, 60, "40M", aux=aux_Z("SA", "c,5,+,10M,60,0;c1,6,-,10M,60,0;c10,7,+,,1,1"))]
    want = same(ctx, tmp_path, recs, chunk=256)
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


@pytest.mark.parametrize("chunk", [4096, 0])
def test_a_cg_record_longer_than_several_chunks(ctx, tmp_path, chunk):
    """the CG:B,I record of tests/test_gpu_bam_walk.py (70 000 ops, 280 KB) between plain records, with an SA tag behind the CG tag"""
    plain = [record(f"p{k}", 0, k % 3, 10 + k, 60, "5S30M", aux=aux_C("NM", k % 5)) for k in range(60)]
    long_rec = bytearray(cg_record())
    tail = aux_Z("SA", SA_OK)
    long_rec = struct.pack("<I", len(long_rec) - 4 + len(tail)) + bytes(long_rec[4:]) + tail
    recs = plain[:30] + [long_rec] + plain[30:]
    want = same(ctx, tmp_path, recs, chunk=chunk)
    assert want[30][6:11] == ["1", "70000", "35000", "0", "0"] and want[30][11:] == ["SA:-1,15,1,40,2,30,0,100"]   # (the record lies on c10 itself)


@pytest.fixture(scope="module")
def random_records(tmp_path_factory):
    """2 000 random records (the size tests/test_gpu_bam_walk.py uses) and the host loader's decode of them, made once"""
    rng = synth.rng_for(20261018)
    pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
    names = [n for n, _ in TARGETS] + ["zzz", "", " c1 "]
    recs = []
    for k in range(2000):
        ops = [(int(rng.integers(0, 31)) << 4) | int(rng.integers(0, 10)) for _ in range(int(rng.integers(0, 41)))]
        name = "".join(chr(int(c)) for c in rng.integers(33, 127, size=int(rng.integers(1, 255))))
        aux = b""
        for _ in range(int(rng.integers(0, 5))):
            kind = int(rng.integers(0, 8))
            if kind == 0:
                ty = pick("cCsSiI")
                lo, hi = {"c": (-128, 128), "C": (0, 256), "s": (-32768, 32768), "S": (0, 65536), "i": (-(1 << 31), 1 << 31), "I": (0, 1 << 32)}[ty]
                aux += aux_t("NM", ty, int(rng.integers(lo, hi)))
            elif kind == 1:
                aux += pick([aux_A("NM", "3"), aux_f("NM", 2.0), aux_Z("NM", "5"), aux_A("SA", "q"), aux_Z("XS", "text"), aux_B("ZB", "s", [1, -2, 3])])
            elif kind in (2, 3):
                items = []
                for _ in range(int(rng.integers(0, 4))):
                    items.append(pick(SA_TEXTS[:-1]) if rng.integers(0, 3) == 0 else "%s,%d,%s,%s,%d,%d" % (
                        pick(names), int(rng.integers(-5, 100000)), pick(["+", "-", ""]), pick(["60S40M", "40M60S", "30S40M30S", "", "5H40M55S", "0S7M"]),
                        int(rng.integers(0, 61)), int(rng.integers(0, 9))))
                aux += aux_Z("SA", ";".join(items) + pick([";", "", ";;"]))
            elif kind == 4:
                aux += b"XQ?" + bytes(int(rng.integers(0, 6)))                            # unknown type: the scan stops here
            else:
                aux += aux_i("AS", int(rng.integers(0, 1000)))
        flag = pick([0, 0, 0, 16, 0x4, 0x100, 0x400, 0x800, 0x41, 0x91])
        recs.append(record(name, flag, int(rng.integers(-1, N_REF + 1)), int(rng.integers(-1, 100000)), int(rng.integers(0, 256)), ops,
                           mtid=int(rng.integers(-1, N_REF)), mpos=int(rng.integers(-1, 100000)), l_seq=int(rng.integers(0, 200)), aux=aux))
    want = host_rows(str(tmp_path_factory.mktemp("bam_columns") / "r.bam"), TARGETS, recs)
    assert len(want) == 2000 and sum(len(w) - 11 for w in want) > 300
    return recs, want


@pytest.mark.parametrize("chunk", [256, 0])
def test_random_records(ctx, random_records, chunk):
    recs, want = random_records
    got, cols = device_rows(ctx, TARGETS, recs, chunk)
    assert len(got) == len(want)
    for i, (w, g) in enumerate(zip(want, got)):
        assert g == w, i
    assert cols["qkey"].tolist() == [name_key(c_name(r), 1) for r in recs]


def names_stream():
    long_a, long_b = "n" * 199 + "a", "n" * 199 + "b"
    nul_a, nul_b = bytearray(record("abXcd", 0, 0, 1, 60, "10M")), bytearray(record("abXxy", 0, 0, 1, 60, "10M"))
    nul_a[36 + 2] = nul_b[36 + 2] = 0
    recs = [record("same", 0, 0, 1, 60, "10M"), record("same", 0x80, 1, 9, 30, "5S5M"), record(long_a, 0, 0, 1, 60, "10M"),
            record(long_b, 0, 0, 1, 60, "10M"), record(long_a, 0, 2, 1, 60, "10M"), record("prefix", 0, 0, 1, 60, "10M"),
            record("prefix_longer", 0, 0, 1, 60, "10M"), bytes(nul_a), bytes(nul_b), record("ab", 0, 0, 1, 60, "10M")]
    stream = header(TARGETS) + b"".join(recs)
    return recs, stream, len(header(TARGETS))


def test_name_keys(ctx):
    recs, stream, first = names_stream()
    starts, _, _ = capi.bam_walk(ctx, stream, first, N_REF)
    assert len(starts) == len(recs)
    for seed in (1, 2):
        assert capi.bam_name_keys(ctx, stream, starts, seed).tolist() == [name_key(c_name(r), seed) for r in recs]
    assert name_key(b"same", 1) != name_key(b"same", 2)


def test_names_differ(ctx):
    recs, stream, first = names_stream()
    starts, _, _ = capi.bam_walk(ctx, stream, first, N_REF)
    differ = lambda pairs: capi.bam_names_differ(ctx, stream, starts, pairs)
    assert differ([(0, 1)]) == 0 and differ([(2, 4)]) == 0 and differ([(3, 3)]) == 0              # equal names
    assert differ([(2, 3)]) == 1                                                                    # the last of 200 bytes
    assert differ([(5, 6)]) == 1 and differ([(6, 5)]) == 1                                          # a common prefix, different lengths
    assert differ([(7, 8)]) == 0 and differ([(7, 9)]) == 0                                          # equal up to an embedded NUL
    assert differ([]) == 0
    pairs = [(0, 1), (2, 3), (2, 4), (5, 6), (7, 8), (0, 9), (1, 0)] * 100                          # more than one wavefront, more than one block
    assert differ(pairs) == 300
