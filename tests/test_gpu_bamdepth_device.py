"""`bamdepth --bam-gpu` (palace_amd/host/bam_stream_device.hpp: the BAM inflated, CRC-checked, walked and decoded on the device)
against the host loader of the same binary: every test runs the same file through both and compares what they print and write.
The kernels themselves: tests/test_gpu_bam_walk.py."""
import gzip
import os
import struct
import subprocess

import pytest

from palace_amd import synth
from tests import graph_cases as gc
from tests.test_host_bam_spec import EOF_MEMBER, bgzf_member, header

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMDEPTH = os.path.join(ROOT, "palace_amd", "bin", "bamdepth")
OPTS = ("PALACE_OPT_BAM_BATCH", "PALACE_OPT_BAM_CHUNK", "PALACE_OPT_DEPTHGZ_BATCH", "PALACE_TRACE")


def run(args, **opts):
    env = {k: v for k, v in os.environ.items() if k not in OPTS}
    env.update({k: str(v) for k, v in opts.items()})
    return subprocess.run([BAMDEPTH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def both(args, bam, **opts):
    """(host loader, --bam-gpu) on the same arguments"""
    return run(args + [bam]), run(["--bam-gpu"] + args + [bam], **opts)


def same_numbers(bam, **opts):
    """default mode and --per-contig: exit status and stdout equal; returns the default mode's stdout"""
    h, g = both([], bam, **opts)
    assert g.returncode == h.returncode, (g.stderr, h.stderr)
    assert g.stdout == h.stdout
    hc, gc_ = both(["--per-contig"], bam, **opts)
    assert gc_.returncode == hc.returncode == 0, (gc_.stderr, hc.stderr)
    assert gc_.stdout == hc.stdout
    return h.stdout


def same_depth_files(tmp_path, bam, tag, **opts):
    """--depth-gz-gpu with and without --bam-gpu: stdout, the .depth.gz and the .tbi byte for byte (both use the device coder)"""
    gz_h, gz_g = str(tmp_path / f"{tag}_h.depth.gz"), str(tmp_path / f"{tag}_g.depth.gz")
    h, g = run(["--depth-gz-gpu", gz_h, bam]), run(["--bam-gpu", "--depth-gz-gpu", gz_g, bam], **opts)
    assert g.returncode == h.returncode == 0, (g.stderr, h.stderr)
    assert g.stdout == h.stdout
    assert open(gz_g, "rb").read() == open(gz_h, "rb").read() and os.path.getsize(gz_g) > 28
    assert open(gz_g + ".tbi", "rb").read() == open(gz_h + ".tbi", "rb").read()


def test_depth_hand_case(tmp_path):
    """the fixture of tests/test_gpu_cli.py::test_bamdepth_hand_case"""
    bam = str(tmp_path / "d.bam")
    synth.write_bam(bam, gc.DEPTH_TARGETS, gc.depth_records())
    h, g = both([], bam)
    assert g.returncode == 0, g.stderr
    assert g.stdout.decode() == gc.DEPTH_TEXT + "\n" == h.stdout.decode()
    synth.write_bam(bam, gc.DEPTH_TARGETS, [synth.BamRecord("u", 4, -1, -1, 0, "")])
    h, g = both([], bam)
    assert g.returncode == h.returncode == 2 and g.stdout == b"" and b"division by zero" in g.stderr


@pytest.fixture(scope="module")
def random_case():
    """the random case of tests/test_gpu_depthgz_device.py: 300 contigs / 20 000 events and its 200 extra records"""
    rng = synth.rng_for(3)
    targets, _, recs, _ = synth.random_graph_case(rng, 300, 20000, long_mode=False)
    extra = []
    for k in range(200):                      # the flags samtools skips, D / N / S / I / = / X, reads over the contig end
        t = int(rng.integers(0, len(targets)))
        L = targets[t][1]
        cig = ["20M5D30M", "10S40M", "25M3I25M2N20M", "30=5X15M", "50M"][k % 5]
        extra.append(synth.BamRecord(f"x{k}", [0, 0x400, 0x100, 0x200, 0x4, 0x800, 16][k % 7], t, int(rng.integers(0, max(1, L - 10))), 60, cig))
    recs = sorted(recs + extra, key=lambda r: (r.tid if r.tid >= 0 else 1 << 30, r.pos))
    return targets, recs


@pytest.mark.parametrize("level", [0, 6])
@pytest.mark.parametrize("block", [300, 4096, 0xFF00])
def test_random_file_equals_the_host_mode(tmp_path, random_case, block, level):
    """records span members at every member size; stored and compressed members"""
    targets, recs = random_case
    bam = str(tmp_path / "r.bam")
    synth.write_bam(bam, targets, recs, block=block, level=level)
    out = same_numbers(bam)
    assert float(out) > 0
    same_depth_files(tmp_path, bam, "r")


def test_small_batch_and_chunk(tmp_path, random_case):
    """two members per batch, chunks of 256 bytes: many batches, records longer than a chunk, the same outputs"""
    targets, recs = random_case
    bam = str(tmp_path / "r.bam")
    synth.write_bam(bam, targets, recs, block=4096, level=6)
    same_numbers(bam, PALACE_OPT_BAM_BATCH=2, PALACE_OPT_BAM_CHUNK=256)
    same_depth_files(tmp_path, bam, "s", PALACE_OPT_BAM_BATCH=2, PALACE_OPT_BAM_CHUNK=256)
    g = run(["--bam-gpu", bam], PALACE_OPT_BAM_BATCH=2, PALACE_OPT_BAM_CHUNK=256, PALACE_TRACE=1)
    line = [l for l in g.stderr.decode().split("\n") if l.startswith("[bamdepth] bam-gpu ms:")]
    assert len(line) == 1
    for lap in ("member index", "header", "upload", "inflate", "crc", "walk", "segments", "chunks", "repaired", "without a start"):
        assert lap in line[0]


def raw_stream(targets, recs):
    return header(targets) + b"".join(r.encode() for r in recs)


def write_members(path, stream, cuts, eof=True, empty_after=()):
    with open(path, "wb") as f:
        for i, (a, b) in enumerate(zip(cuts, cuts[1:])):
            f.write(bgzf_member(stream[a:b]))
            if i in empty_after:
                f.write(bgzf_member(b""))
        if eof:
            f.write(EOF_MEMBER)


def small_case(n_targets=5, n_recs=400, name="ctg_{}"):
    targets = [(name.format(t), 2000 + 10 * t) for t in range(n_targets)]
    recs = [synth.BamRecord(f"r{k}", 0, k * n_targets // n_recs, (k * 37) % 1900, 60, ["50M", "10S30M5D20M", "20=2X20M"][k % 3]) for k in range(n_recs)]
    return targets, recs


def test_member_edge_cases(tmp_path):
    targets, recs = small_case()
    stream = raw_stream(targets, recs)
    cuts = list(range(0, len(stream), 5000)) + [len(stream)]
    bam = str(tmp_path / "e.bam")
    write_members(bam, stream, cuts)
    want = same_numbers(bam)
    assert float(want) > 1
    write_members(bam, stream, cuts, eof=False)                               # no EOF member
    assert same_numbers(bam) == want
    write_members(bam, stream, cuts, empty_after=(0, 1, 3))                   # empty members in the middle
    assert same_numbers(bam) == want
    write_members(bam, stream, [0, 3, 90, 91, 200, 333, len(stream) - 2, len(stream)], eof=False, empty_after=(3,))
    assert same_numbers(bam) == want
    # a header larger than one member: 3 000 targets whose names make it longer than any member can be (28 bytes apiece, 84 KB)
    targets, recs = small_case(3000, 3000, name="ctg_{:05d}_of_assembly")
    stream = raw_stream(targets, recs)
    assert len(header(targets)) > 65536
    write_members(bam, stream, list(range(0, len(stream), 0xff00)) + [len(stream)])
    assert float(same_numbers(bam)) > 0
    same_depth_files(tmp_path, bam, "big")


def rejected_like_the_host(tmp_path, bam):
    """same exit status as the host mode, nothing on stdout, one stderr line naming the file, no output file"""
    for args in ([], ["--per-contig"]):
        h, g = both(args, bam)
        assert g.returncode == h.returncode == 1 and g.stdout == b"" and h.stdout == b""
        assert g.stderr.count(b"\n") == 1 and bam.encode() in g.stderr
    gz_h, gz_g = str(tmp_path / "bad_h.depth.gz"), str(tmp_path / "bad_g.depth.gz")
    h, g = run(["--depth-gz-gpu", gz_h, bam]), run(["--bam-gpu", "--depth-gz-gpu", gz_g, bam])
    assert g.returncode == h.returncode == 1 and g.stdout == b""
    assert not os.path.exists(gz_g) and not os.path.exists(gz_g + ".tbi")


def test_damaged_files(tmp_path):
    """a member whose DEFLATE data are damaged, a truncated last member, gzip that is not BGZF, BGZF that is not BAM"""
    targets, recs = small_case()
    bam = str(tmp_path / "x.bam")
    synth.write_bam(bam, targets, recs, block=4096, level=0)
    good = open(bam, "rb").read()
    second = struct.unpack_from("<H", good, 16)[0] + 1                        # the second member: 18 bytes of header, a stored block
    assert good[second + 18] & 7 == 1                                         # BFINAL, BTYPE 00: LEN and NLEN follow
    # ... its NLEN flipped: no decoder takes the member
    open(bam, "wb").write(good[:second + 21] + bytes([good[second + 21] ^ 0x10]) + good[second + 22:])
    rejected_like_the_host(tmp_path, bam)
    # truncated inside the last data member
    last = len(good) - 28
    open(bam, "wb").write(good[:last - 40])
    rejected_like_the_host(tmp_path, bam)
    open(bam, "wb").write(gzip.compress(b"@HD\tVN:1.6\n" * 50))
    rejected_like_the_host(tmp_path, bam)
    open(bam, "wb").write(bgzf_member(b"not a BAM at all, " * 20) + EOF_MEMBER)
    rejected_like_the_host(tmp_path, bam)


def test_a_flipped_data_byte_is_caught_by_the_crc(tmp_path):
    """one byte of a stored member's data flipped: the DEFLATE stream is intact, only the CRC-32 of the trailer tells.  The device mode
    compares every member's CRC-32 (palace_crc32_members) and rejects the file; the host loader never checked CRCs and is not
    compared here"""
    targets, recs = small_case()
    bam = str(tmp_path / "x.bam")
    synth.write_bam(bam, targets, recs, block=4096, level=0)
    good = open(bam, "rb").read()
    second = struct.unpack_from("<H", good, 16)[0] + 1
    at = second + 18 + 5 + 1000
    open(bam, "wb").write(good[:at] + bytes([good[at] ^ 0x01]) + good[at + 1:])
    gz = str(tmp_path / "crc.depth.gz")
    for args in ([bam], ["--depth-gz-gpu", gz, bam]):
        g = run(["--bam-gpu"] + args)
        assert g.returncode == 1 and g.stdout == b"" and b"CRC-32" in g.stderr and bam.encode() in g.stderr and g.stderr.count(b"\n") == 1
    assert not os.path.exists(gz)


def test_malformed_record_mid_file(tmp_path):
    """l_read_name 0 in record 250 of 400: the stream ends there for both loaders"""
    targets, recs = small_case()
    enc = [r.encode() for r in recs]
    bad = bytearray(enc[250])
    bad[4 + 8] = 0
    stream = header(targets) + b"".join(enc[:250]) + bytes(bad) + b"".join(enc[251:])
    bam = str(tmp_path / "m.bam")
    write_members(bam, stream, list(range(0, len(stream), 3000)) + [len(stream)])
    cut = same_numbers(bam)
    write_members(bam, header(targets) + b"".join(enc[:250]), [0, len(header(targets)) + sum(len(e) for e in enc[:250])])
    assert same_numbers(bam) == cut                                           # ... and is the file of the records in front of it
    write_members(bam, header(targets) + b"".join(enc), [0, len(header(targets)) + sum(len(e) for e in enc)])
    assert same_numbers(bam) != cut
