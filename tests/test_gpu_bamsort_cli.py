"""The `bamsort` executable end to end on BAM files built here byte by byte (tests/test_host_bam_spec.py's builders, tests/gz_util.py):
the file it writes is read back member by member with zlib and must be the rewritten header + the stably sorted records; the .bai is
read by the spec-derived tests/bai_reader.py and must answer region queries exactly.  Expectations come from the Python restatement of
tests/bam_sort_cases.py, never from the device."""
import os
import random
import struct
import subprocess

import pytest

from tests import bai_cases as bai
from tests import bam_sort_cases as bc
from tests import gz_util
from tests.bai_reader import PSEUDO_BIN, IndexedBam, read_bai
from tests.tabix_reader import EOF_MEMBER, bgzf_members
from tests.test_host_bam_spec import aux_Z, header, record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
BAMSORT, BAMDEPTH, HOSTDUMP = (os.path.join(BIN, n) for n in ("bamsort", "bamdepth", "hostdump"))
MEMBER = 0xff00
TARGETS = [("c0", 300000), ("c1", 5000), ("empty", 1000), ("big", (1 << 29) - 1), ("c4", 70000)]


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host")] + [os.path.join("..", "bin", n) for n in ("bamsort", "bamdepth", "hostdump")],
                   check=True, stdout=subprocess.DEVNULL)


def run(args, env=None, tool=BAMSORT):
    return subprocess.run([tool] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **(env or {})), timeout=120)


def sort_ok(args, env=None):
    p = run(args, env)
    assert p.returncode == 0 and p.stdout == b"" and p.stderr == b"", p.stderr.decode()


def expected_stream(text, targets, recs):
    return header(targets, bc.rewrite_text(text)) + b"".join(bc.sorted_records(recs, len(targets)))


def read_sorted(path, want):
    """the file member by member (each checked by the reader: BSIZE, CRC-32, ISIZE) -> its members; the stream must be `want`"""
    data = open(path, "rb").read()
    mem = bgzf_members(data)
    assert data[-28:] == EOF_MEMBER and mem[-1][1] == b""
    sizes = [len(x) for _, x in mem[:-1]]
    assert all(s == MEMBER for s in sizes[:-1]) and (not sizes or 0 < sizes[-1] <= MEMBER)
    got = b"".join(x for _, x in mem)
    assert len(got) == len(want) and got == want
    return mem


# ---- one file with every shape the index has to get right, sorted and indexed once -------------------------------------------
def main_records():
    rng = random.Random(77)
    recs = bc.random_records(rng, 2600, TARGETS[:2] + TARGETS[4:], unplaced=0.04)
    for k, r in enumerate(recs):                                             # (the generator's third target is c4: refID 4)
        f = bc.fields(r)
        if f["tid"] == 2:
            recs[k] = r[:4] + struct.pack("<i", 4) + r[8:]
    end = (1 << 29) - 1
    recs += [record("at_the_end", 0, 3, end - 100, 60, "100M"), record("big_start", 16, 3, 0, 60, "30M"), record("big_mid", 0, 3, 1 << 28, 60, "10M5000N10M"),
             bc.cg_record("cg_long", 0, 0, 150000, "5S" + "2M1D" * 300 + "20M"), record("mate_unmapped", 4 | 1 | 64, 0, 16384, 0, "", l_seq=20, mtid=0, mpos=16384),
             record("window_edge", 0, 0, 16383, 60, "2M"), record("window_edge2", 0, 0, 32768, 60, "1M")]
    rng.shuffle(recs)
    return recs


@pytest.fixture(scope="module")
def main_case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamsort_main")
    recs = main_records()
    n_ref = len(TARGETS)
    srt = bc.sorted_records(recs, n_ref)
    # an @CO line pads the header so that a sorted record starts exactly on a member boundary ...
    base = len(header(TARGETS, bc.rewrite_text("@HD\tVN:1.6\tSO:unsorted\n@CO\t\n")))
    cum, k = base, 0
    while cum + len(srt[k]) <= MEMBER:
        cum += len(srt[k])
        k += 1
    text = "@HD\tVN:1.6\tSO:unsorted\n@CO\t" + "p" * (MEMBER - cum) + "\n"
    # ... and a last unplaced record makes the stream end exactly on one
    so_far = len(expected_stream(text, TARGETS, recs))
    tail = record("tail", 4, -1, -1, 0, "", l_seq=0, aux=aux_Z("XT", "t" * ((-(so_far + 4 + 32 + 5 + 4)) % MEMBER)))
    recs.append(tail)
    want = expected_stream(text, TARGETS, recs)
    assert len(want) % MEMBER == 0 and len(want) >= 3 * MEMBER
    src, out = tmp / "in.bam", tmp / "out.bam"
    src.write_bytes(gz_util.bgzf(header(TARGETS, text) + b"".join(recs)))
    sort_ok(["-@", 4, src, "-O", "BAM", "-o", out, "--bai"])
    return dict(tmp=tmp, src=src, out=out, recs=recs, text=text, want=want, boundary_record=k)


def test_sorted_file_is_header_and_stably_sorted_records(main_case):
    mem = read_sorted(main_case["out"], main_case["want"])
    assert len(mem) >= 4
    ib = IndexedBam(main_case["out"])
    assert ib.text.decode() == bc.rewrite_text(main_case["text"]) and ib.targets == TARGETS
    offs = [at for at, _ in ib.records]
    assert MEMBER in offs and offs.index(MEMBER) == main_case["boundary_record"]          # a record starts exactly on a member boundary
    assert sorted(os.listdir(main_case["tmp"])) == ["in.bam", "out.bam", "out.bam.bai"]


def test_index_structure(main_case):
    ib = IndexedBam(main_case["out"])
    n_ref = len(TARGETS)
    srt = [r for _, r in ib.records]
    assert ib.bai["n_no_coor"] == sum(1 for r in srt if bc.fields(r)["tid"] < 0) > 0
    assert len(ib.bai["refs"]) == n_ref
    rec_end = {at: at + len(r) for at, r in ib.records}
    for tid, ref in enumerate(ib.bai["refs"]):
        mine = [(at, r) for at, r in ib.records if bc.fields(r)["tid"] == tid]
        if not mine:
            assert ref["bins"] == {} and ref["ioff"] == [] and TARGETS[tid][0] == "empty"
            continue
        assert ref["order"][-1] == PSEUDO_BIN and ref["order"][:-1] == sorted(ref["order"][:-1])           # bins increasing, the pseudo-bin last
        (p_beg, p_end), (n_map, n_un) = ref["bins"][PSEUDO_BIN]
        assert (ib.abs(p_beg), ib.abs(p_end)) == (mine[0][0], rec_end[mine[-1][0]])
        assert (n_map, n_un) == (sum(1 for _, r in mine if not bc.fields(r)["flag"] & 4), sum(1 for _, r in mine if bc.fields(r)["flag"] & 4))
        # the chunks are exactly the maximal runs of equal bin, in file order within a bin
        runs = {}
        for at, r in mine:
            b = bc.reg2bin(*bc.span(r))
            if runs.get("last") == b:
                runs[b][-1][1] = rec_end[at]
            else:
                runs.setdefault(b, []).append([at, rec_end[at]])
            runs["last"] = b
        del runs["last"]
        got = {b: [[ib.abs(cb), ib.abs(ce)] for cb, ce in ch] for b, ch in ref["bins"].items() if b != PSEUDO_BIN}
        assert got == runs
        flat = sorted(c for ch in got.values() for c in ch)
        assert all(a[1] <= b[0] for a, b in zip(flat, flat[1:]))                                              # non-overlapping
        assert all(ib.voff_is_canonical(v) for b, ch in ref["bins"].items() if b != PSEUDO_BIN for c in ch for v in c)
        assert ib.voff_is_canonical(p_beg) and ib.voff_is_canonical(p_end)
        # the linear index
        ends = [(bc.span(r)[1] - 1) >> 14 for _, r in mine]
        assert len(ref["ioff"]) == 1 + max(ends)
        want, nxt = [None] * len(ref["ioff"]), None
        for at, r in mine:
            b, e = bc.span(r)
            for w in range(b >> 14, ((e - 1) >> 14) + 1):
                want[w] = at if want[w] is None else min(want[w], at)
        for w in range(len(want) - 1, -1, -1):
            if want[w] is None:
                want[w] = nxt
            nxt = want[w]
        assert [ib.abs(v) for v in ref["ioff"]] == want
    last = ib.records[-1]
    assert rec_end[last[0]] == len(ib.stream) and len(ib.stream) % MEMBER == 0                                # the last record ends on a boundary


def test_region_queries_are_exact_with_and_without_the_linear_index(main_case):
    ib = IndexedBam(main_case["out"])
    rng = random.Random(3)
    regions = []
    for _ in range(200):
        tid = rng.choice((0, 0, 0, 1, 3, 4, 2))
        tlen = TARGETS[tid][1]
        beg = rng.randrange(tlen)
        regions.append((tid, beg, min(tlen, beg + rng.choice((1, 10, 1000, 20000, 200000, tlen)))))
    for tid in (0, 4):
        for edge in range(16384, TARGETS[tid][1], 16384):
            regions += [(tid, edge - 1, edge), (tid, edge, edge + 1), (tid, edge - 1, edge + 1)]
    end = (1 << 29) - 1
    regions += [(3, end - 1, end), (3, end - 100, end - 99), (3, end - 101, end - 100), (3, 0, end), (3, (1 << 28) + 2000, (1 << 28) + 2001), (0, 0, 300000)]
    hits = 0
    for tid, beg, e in regions:
        want = ib.brute(tid, beg, e)
        assert ib.fetch(tid, beg, e) == want, (tid, beg, e)
        assert ib.fetch(tid, beg, e, use_linear=False) == want, (tid, beg, e)
        hits += len(want)
    assert hits > 1000


def test_bai_equals_index_of_the_written_file(main_case):
    other = main_case["tmp"] / "other.bai"
    sort_ok(["--index", main_case["out"], other])
    assert other.read_bytes() == (main_case["tmp"] / "out.bam.bai").read_bytes()
    os.remove(other)


def test_sorting_the_output_again_gives_the_same_stream(main_case):
    again = main_case["tmp"] / "again.bam"
    sort_ok(["-o", again, main_case["out"]])
    read_sorted(again, main_case["want"])
    os.remove(again)


def test_batch_size_does_not_change_the_file(main_case):
    tmp = main_case["tmp"]
    for batch in ("1", "3"):
        other = tmp / f"batch{batch}.bam"
        sort_ok(["-o", other, "--bai", main_case["src"]], env={"PALACE_OPT_BAMSORT_BATCH": batch, "PALACE_OPT_BAM_BATCH": "2"})
        assert other.read_bytes() == main_case["out"].read_bytes()
        assert (tmp / f"batch{batch}.bam.bai").read_bytes() == (tmp / "out.bam.bai").read_bytes()
        os.remove(other)
        os.remove(tmp / f"batch{batch}.bam.bai")


def test_host_loader_reads_the_device_coders_members(main_case):
    """bamdepth and hostdump agree on the output and on a Python-sorted, zlib-written twin"""
    twin = main_case["tmp"] / "twin.bam"
    twin.write_bytes(gz_util.bgzf(main_case["want"]))
    for tool, args in ((BAMDEPTH, []), (HOSTDUMP, ["bam"])):
        a, b = run(args + [main_case["out"]], tool=tool), run(args + [twin], tool=tool)
        assert a.returncode == b.returncode == 0 and a.stdout == b.stdout and len(a.stdout) > 0, (a.stderr, b.stderr)
    os.remove(twin)


# ---- headers, input shapes, errors: small files ----------------------------------------------------------------------------------
SMALL_TARGETS = [("t0", 5000), ("t1", 900)]


def small_records(seed=1, n=300):
    return bc.random_records(random.Random(seed), n, SMALL_TARGETS)


@pytest.mark.parametrize("text", ["@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:t0\tLN:5000\n", "@HD\tVN:1.5\tGO:none\n@CO\tSO:unsorted stays\n", "@HD\tVN:1.6\tSO:queryname\tSS:x",
                                  "@SQ\tSN:t0\tLN:5000\n@PG\tID:bwa\n", ""])
def test_header_cases(tmp_path, text):
    recs = small_records()
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(gz_util.bgzf(header(SMALL_TARGETS, text) + b"".join(recs)))
    sort_ok(["-o", out, src])
    read_sorted(out, expected_stream(text, SMALL_TARGETS, recs))
    ib_text = bc.rewrite_text(text)
    assert ib_text.split("\n")[0].count("SO:coordinate") == 1 and "@PG\tID:bamsort" not in ib_text
    assert not os.path.exists(str(out) + ".bai")


@pytest.mark.parametrize("shape", ["stored", "level6", "three_members", "no_eof", "empty"])
def test_input_shapes(tmp_path, shape):
    text = "@HD\tVN:1.6\n"
    recs = [] if shape == "empty" else small_records(seed=5)
    if shape == "three_members":
        recs.insert(40, record("wide", 0, 0, 77, 60, "50M", aux=aux_Z("XW", "w" * 150000)))
    stream = header(SMALL_TARGETS, text) + b"".join(recs)
    blob = {"stored": lambda: gz_util.bgzf(stream, level=0), "level6": lambda: gz_util.bgzf(stream, level=6), "empty": lambda: gz_util.bgzf(stream),
            "three_members": lambda: gz_util.bgzf(stream, block=60000), "no_eof": lambda: gz_util.bgzf(stream, block=7000, eof=False)}[shape]()
    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(blob)
    sort_ok(["-o", out, src, "--bai"])
    read_sorted(out, expected_stream(text, SMALL_TARGETS, recs))
    ib = IndexedBam(out)
    for tid in range(len(SMALL_TARGETS)):
        assert ib.fetch(tid, 0, SMALL_TARGETS[tid][1]) == ib.brute(tid, 0, SMALL_TARGETS[tid][1])
    if shape == "empty":
        assert read_bai(str(out) + ".bai") == dict(refs=[dict(bins={}, order=[], ioff=[])] * 2, n_no_coor=0)


def test_errors_leave_no_file(tmp_path):
    recs = small_records(seed=6, n=50)
    good = header(SMALL_TARGETS) + b"".join(recs)
    cases = {"tail": (good + b"\x05\0\0\0ab", b"malformed record at offset " + str(len(good)).encode()),
             "tid": (good[:0] + header(SMALL_TARGETS) + b"".join(recs[:7] + [record("x", 0, 2, 5, 0, "5M")] + recs[7:]), b"record 7:"),
             "pos": (header(SMALL_TARGETS) + b"".join(recs[:11] + [record("x", 0, 1, -2, 0, "5M")] + recs[11:]), b"record 11:")}
    for name, (stream, message) in cases.items():
        src, out = tmp_path / f"{name}.bam", tmp_path / f"{name}.sorted.bam"
        src.write_bytes(gz_util.bgzf(stream))
        p = run(["-o", out, "--bai", src])
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"bamsort: ") and message in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
        assert not os.path.exists(out) and not os.path.exists(str(out) + ".bai")


def test_index_of_a_zlib_written_file_with_other_members(tmp_path):
    recs = small_records(seed=8, n=900)
    stream = expected_stream("@HD\tVN:1.6\n", SMALL_TARGETS, recs)
    bam = tmp_path / "sorted.bam"
    for eof in (True, False):
        bam.write_bytes(gz_util.bgzf(stream, block=4000, eof=eof))
        sort_ok(["--index", bam])
        ib = IndexedBam(bam)
        assert len(ib.members) > 10
        for tid in range(2):
            for beg in range(0, SMALL_TARGETS[tid][1], 397):
                assert ib.fetch(tid, beg, beg + 200) == ib.brute(tid, beg, beg + 200)
                assert ib.fetch(tid, beg, beg + 200, use_linear=False) == ib.brute(tid, beg, beg + 200)
        assert ib.bai["n_no_coor"] == sum(1 for r in recs if bc.fields(r)["tid"] < 0)


def test_index_refuses_an_unsorted_file_and_records_a_bai_cannot_hold(tmp_path):
    recs = bc.sorted_records(small_records(seed=9, n=200), 2)
    swapped = recs[:]
    k = next(i for i in range(len(recs) - 1) if bc.sort_key(recs[i], 2) < bc.sort_key(recs[i + 1], 2) and i > 20)
    swapped[k], swapped[k + 1] = swapped[k + 1], swapped[k]
    minus = [record("m", 0, 0, -1, 0, "5M")] + recs
    for name, rs, message in (("unsorted", swapped, f"is not coordinate-sorted (record {k + 1})".encode()), ("minus", minus, b"record 0: outside what a .bai can index")):
        bam = tmp_path / f"{name}.bam"
        bam.write_bytes(gz_util.bgzf(header(SMALL_TARGETS) + b"".join(rs)))
        p = run(["--index", bam])
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"bamsort: ") and message in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
        assert not os.path.exists(str(bam) + ".bai")


# ---- more targets than 16 bits count: the index's per-reference kernels and run keys in the executable ------------------------------
def test_seventy_thousand_targets(tmp_path):
    """records on the references around 256 and 65 536 and on 900 others of 70 000, most references without any: the run key's reference
    bits above 16 and several workgroups of the per-reference kernels, through the executable"""
    n_ref, tlen = 70000, 100000
    targets = [(f"t{k}", tlen) for k in range(n_ref)]
    recs, used = bai.many_reference_records(random.Random(70), n_ref, 900, tlen, 25)
    assert 3000 < len(recs) < 5500 and {65535, 65536, 65537} <= set(used)
    text = "@HD\tVN:1.6\tSO:unsorted\n"

    def head(t):                                                            # (header() appends target by target: too slow for 70 000)
        return b"BAM\1" + struct.pack("<i", len(t)) + t.encode() + struct.pack("<i", n_ref) + b"".join(
            struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", l) for n, l in targets)

    src, out = tmp_path / "in.bam", tmp_path / "out.bam"
    src.write_bytes(gz_util.bgzf(head(text) + b"".join(recs), level=1))
    sort_ok(["-o", out, "--bai", src])
    read_sorted(out, head(bc.rewrite_text(text)) + b"".join(bc.sorted_records(recs, n_ref)))
    ib = IndexedBam(out)
    assert ib.targets == targets and len(ib.bai["refs"]) == n_ref and ib.bai["n_no_coor"] == 25
    rng = random.Random(71)
    empty = [t for t in (2, 254, 2000, 2999, 65534, 65538, 66000, 66999, 69998) + tuple(rng.sample(range(n_ref), 12)) if t not in used]
    assert len(empty) >= 8
    for tid in empty:
        assert ib.bai["refs"][tid] == dict(bins={}, order=[], ioff=[]) and ib.fetch(tid, 0, tlen) == ib.brute(tid, 0, tlen) == []
    hits = 0
    for tid in list(bai.FORCED_REFS) + rng.sample(used, 10):
        for beg, end in ((0, tlen), (16383, 16385), (40000, 60000), (rng.randrange(tlen), tlen)):
            want = ib.brute(tid, beg, end)
            assert ib.fetch(tid, beg, end) == want and ib.fetch(tid, beg, end, use_linear=False) == want, (tid, beg, end)
            hits += len(want)
    assert hits > 150
    other = tmp_path / "other.bai"
    sort_ok(["--index", out, other])
    assert other.read_bytes() == (tmp_path / "out.bam.bai").read_bytes()
