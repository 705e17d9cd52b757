"""`bamsort --lz`, `bamsort --sam --lz` and `samview --lz` end to end: the members come from palace_bgzf_deflate_lz, everything else is
the unflagged run's.  On the inputs of tests/bamsort_lz_cases.py the flagged file inflates, member by member with zlib, to exactly the
stream the unflagged run writes (and the Python restatement expects); its members hold match tokens and are fewer bytes in all; its
.bai is the index of the file that was written and answers region queries like brute force; `bamdepth` reads both files alike; and
`--lz` with `-u` is a usage error."""
import os
import random
import subprocess

import pytest

from tests import bamsort_lz_cases as cl
from tests import deflate_lz_model as lz
from tests import gz_util
from tests.bai_reader import IndexedBam
from tests.tabix_reader import EOF_MEMBER, bgzf_members

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
SAMVIEW, BAMSORT, BAMDEPTH = (os.path.join(BIN, n) for n in ("samview", "bamsort", "bamdepth"))


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host")] + [os.path.join("..", "bin", n) for n in ("samview", "bamsort", "bamdepth")],
                   check=True, stdout=subprocess.DEVNULL)


def run(tool, args, stdin=b""):
    return subprocess.run([tool] + [str(a) for a in args], input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def ok(tool, args, stdin=b""):
    p = run(tool, args, stdin)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode()
    return p.stdout


def texts(data):
    """the file's members (BSIZE, CRC-32 and ISIZE checked by the reader) -> their texts, the EOF member's last"""
    mem = bgzf_members(data)
    assert data[-28:] == EOF_MEMBER and mem[-1][1] == b""
    return [x for _, x in mem]


def members(data):
    mem = bgzf_members(data)
    return [data[a:b] for (a, _), (b, _) in zip(mem[:-1], mem[1:])]


def same_stream_fewer_bytes(flagged, plain, want):
    """the flagged file against the unflagged one: the same texts member by member, matches in its members, fewer bytes in all"""
    assert texts(flagged) == texts(plain) and b"".join(texts(flagged)) == want
    mine = members(flagged)
    assert len(mine) >= 5 and all(len(m) <= cl.MEMBER + 31 for m in mine)
    assert any(lz.has_match(m) for m in mine)
    print(f"{len(want)} bytes of stream: --lz {len(flagged)}, without {len(plain)}")
    assert len(flagged) < len(plain)


@pytest.fixture(scope="module")
def sorted_case(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bamsort_lz")
    stream, want = cl.bam_case()
    (tmp / "in.bam").write_bytes(gz_util.bgzf(stream))
    assert ok(BAMSORT, ["-@", 4, tmp / "in.bam", "-O", "BAM", "-o", tmp / "plain.bam", "--bai"]) == b""
    assert ok(BAMSORT, ["-@", 4, "--lz", tmp / "in.bam", "-O", "BAM", "-o", tmp / "lz.bam", "--bai"]) == b""
    return dict(tmp=tmp, want=want)


def test_bamsort_lz_writes_the_same_stream_in_fewer_bytes(sorted_case):
    tmp = sorted_case["tmp"]
    same_stream_fewer_bytes((tmp / "lz.bam").read_bytes(), (tmp / "plain.bam").read_bytes(), sorted_case["want"])


def test_its_bai_is_the_index_of_the_written_file_and_answers_region_queries(sorted_case):
    tmp = sorted_case["tmp"]
    assert ok(BAMSORT, ["--index", tmp / "lz.bam", tmp / "other.bai"]) == b""
    assert (tmp / "other.bai").read_bytes() == (tmp / "lz.bam.bai").read_bytes()
    assert (tmp / "lz.bam.bai").read_bytes() != (tmp / "plain.bam.bai").read_bytes()      # (other members, other file offsets)
    ib = IndexedBam(tmp / "lz.bam")
    assert ib.targets == cl.TARGETS
    rng, hits = random.Random(4), 0
    regions = [(tid, 0, tlen) for tid, (_, tlen) in enumerate(cl.TARGETS)] + [(0, 16383, 16385), (2, 32767, 32769)]
    for _ in range(120):
        tid = rng.randrange(len(cl.TARGETS))
        tlen = cl.TARGETS[tid][1]
        beg = rng.randrange(tlen)
        regions.append((tid, beg, min(tlen, beg + rng.choice((1, 100, 5000, 100000)))))
    for tid, beg, end in regions:
        want = ib.brute(tid, beg, end)
        assert ib.fetch(tid, beg, end) == want and ib.fetch(tid, beg, end, use_linear=False) == want, (tid, beg, end)
        hits += len(want)
    assert hits > 1000


def test_bamdepth_reads_both_files_alike(sorted_case):
    tmp = sorted_case["tmp"]
    for args in ([], ["--per-contig"]):
        a, b = ok(BAMDEPTH, args + [tmp / "lz.bam"]), ok(BAMDEPTH, args + [tmp / "plain.bam"])
        assert a == b and len(a) > 0


def test_the_batch_size_does_not_change_the_file(sorted_case):
    tmp = sorted_case["tmp"]
    p = subprocess.run([BAMSORT, "--lz", "-o", str(tmp / "b2.bam"), "--bai", str(tmp / "in.bam")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, PALACE_OPT_BAMSORT_BATCH="2"), timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode()
    assert (tmp / "b2.bam").read_bytes() == (tmp / "lz.bam").read_bytes() and (tmp / "b2.bam.bai").read_bytes() == (tmp / "lz.bam.bai").read_bytes()


def test_samview_lz_and_bamsort_sam_lz(tmp_path):
    text, want = cl.sam_case()
    sam = tmp_path / "in.sam"
    sam.write_bytes(text)
    assert ok(SAMVIEW, ["-F", "0x0800", "-bS", "-o", tmp_path / "plain.bam", sam]) == b""
    assert ok(SAMVIEW, ["-F", "0x0800", "-bS", "--lz", "-o", tmp_path / "lz.bam", sam]) == b""
    flagged = (tmp_path / "lz.bam").read_bytes()
    same_stream_fewer_bytes(flagged, (tmp_path / "plain.bam").read_bytes(), want)
    assert ok(SAMVIEW, ["--lz", "-F", "0x0800", "-b", "-"], text) == flagged                        # to stdout, from stdin
    a, b = ok(BAMDEPTH, [tmp_path / "lz.bam"]), ok(BAMDEPTH, [tmp_path / "plain.bam"])
    assert a == b and len(a) > 0
    # bamsort --sam --lz: what bamsort --lz makes of samview's output, and the unflagged run's stream
    assert ok(BAMSORT, ["--sam", "-F", "0x0800", sam, "-o", tmp_path / "one.bam", "--bai", "--lz"]) == b""
    assert ok(BAMSORT, ["--lz", tmp_path / "plain.bam", "-o", tmp_path / "two.bam", "--bai"]) == b""
    assert ok(BAMSORT, ["--sam", "-F", "0x0800", sam, "-o", tmp_path / "three.bam", "--bai"]) == b""
    one = (tmp_path / "one.bam").read_bytes()
    assert one == (tmp_path / "two.bam").read_bytes() and (tmp_path / "one.bam.bai").read_bytes() == (tmp_path / "two.bam.bai").read_bytes()
    three = (tmp_path / "three.bam").read_bytes()
    same_stream_fewer_bytes(one, three, b"".join(texts(three)))
    assert ok(BAMSORT, ["--index", tmp_path / "one.bam", tmp_path / "other.bai"]) == b""
    assert (tmp_path / "other.bai").read_bytes() == (tmp_path / "one.bam.bai").read_bytes()


def test_lz_with_u_is_a_usage_error(tmp_path):
    sam = tmp_path / "in.sam"
    sam.write_bytes(cl.sam_case()[0])
    for args in (["-bu", "--lz", sam], ["--lz", "-b", "-u", "-o", tmp_path / "out.bam", sam]):
        p = run(SAMVIEW, args)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"Usage: samview"), p.stderr
    assert sorted(os.listdir(tmp_path)) == ["in.sam"]
