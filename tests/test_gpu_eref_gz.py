"""eref on gzip-compressed FASTQ: the device FASTQ parser at the C ABI against the getline model, the member CRC-32 kernel against
zlib, and the eref executable on BGZF / gzip / mixed inputs against the reference's goldens and against its own plain-text path."""
import gzip
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

from oracle import binding as orc
from palace_amd import capi, synth
from tests import gz_util as gz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


# ------------------------------------------------------------------------------------------------
# host-only: the writers produce what gzip reads
# ------------------------------------------------------------------------------------------------
def test_writers_round_trip():
    data = bytes(np.random.default_rng(5).integers(0, 256, size=200_000, dtype=np.uint8))
    for blob in (gz.bgzf(data, 4000), gz.bgzf(data, level=0), gz.gzip_members(data, [1, 7777, 150_001]),
                 gz.gzip_member(data, fname=b"r_1.fq", comment=b"c", extra=b"XY\x02\x00ab", hcrc=True)):
        assert gzip.decompress(blob) == data
    assert gz.model_read_set(b"") == (b"", [0])
    assert gz.model_read_set(b"@a\nACG\n+\nIII") == (b"ACG", [0, 3])
    assert gz.model_read_set(b"@a\n\n+\n\n@b\nT") == (b"T", [0, 0, 1])


# ------------------------------------------------------------------------------------------------
# 1. the parser at the C ABI
# ------------------------------------------------------------------------------------------------
def adversarial_text(rng, n_records=400):
    parts = []
    lens = [0, 1, 31, 32, 33, 65]
    for i in range(n_records):
        L = lens[i % len(lens)] if i < 60 else int(rng.integers(0, 300))
        alphabet = np.frombuffer(b"ACGTacgtNn\r\x80\xff", dtype=np.uint8)
        seq = bytes(rng.choice(alphabet, size=L)) if i % 5 == 0 else bytes(rng.choice(alphabet[:4], size=L))
        hdr = b"@r%d" % i + (b"\r" if i % 7 == 0 else b"")
        parts.append(hdr + b"\n" + seq + (b"\r\n" if i % 11 == 0 else b"\n") + b"+\n" + b"I" * L + b"\n")
        if i % 37 == 0:
            parts.append(b"\n")                                    # a blank line shifts every later line's phase
    return b"".join(parts)


def check_parse(ctx, text, cuts=(), reads0=0, bases0=0):
    want_b, want_o = gz.model_read_set(text)
    b, o, cur = capi.fastq_read_set(ctx, text, cuts, reads0, bases0)
    assert b.tobytes() == want_b
    assert o.tolist() == [bases0 + x for x in want_o]
    assert int(cur["reads"]) == reads0 + len(want_o) - 1 and int(cur["bases"]) == bases0 + len(want_b)


@pytest.mark.gpu
def test_parser_equals_getline_model_on_adversarial_text():
    rng = np.random.default_rng(11)
    with capi.Ctx(0) as ctx:
        for text in (b"", b"\n", b"\n\n", b"@a", b"@a\n", b"@a\nACGT", b"@a\nACGT\n", b"@a\n\n+\n\n", b"@a\r\nAC\r\n+\r\nII\r\n",
                     b"\n" * 9 + b"x", b"@a\nA\n+\nI\n@b\nCC\n+\nII"):
            check_parse(ctx, text)
            check_parse(ctx, text, reads0=3, bases0=17)            # a second file behind an earlier one
        text = adversarial_text(rng)
        check_parse(ctx, text)
        check_parse(ctx, text + b"@z\nACGTN")                        # no final newline
        small = text[:300]
        for c in range(0, len(small) + 1):                         # every cut of a small case into two windows
            check_parse(ctx, small, [c])
        for _ in range(12):                                        # random cuts of a large case (windows of 1 .. 60 000 bytes)
            cuts = sorted(set(int(x) for x in rng.integers(0, len(text), size=int(rng.integers(1, 60)))))
            check_parse(ctx, text, cuts)
        # a line longer than the window (and longer than anything else in the file), and a file that is one line
        big = b"@long\n" + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=300_000)) + b"\n+\n" + b"I" * 300_000 + b"\n"
        check_parse(ctx, big + text, list(range(4096, len(big) + len(text), 4096)))
        check_parse(ctx, b"A" * 100_000, list(range(1000, 100_000, 1000)))
        check_parse(ctx, b"@x\n" + b"G" * 100_003, list(range(16, 100_006, 16 * 997)))


@pytest.mark.gpu
def test_parser_read_set_counts_like_host_read_set(golden_eref):
    g = golden_eref
    r1 = synth.ReadSet(g["r1_bases"], g["r1_offsets"])
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        r1.write_fastq(os.path.join(d, "a.fq"), "1")
        text = open(os.path.join(d, "a.fq"), "rb").read()
    with capi.Ctx(0) as ctx:
        b, o, _ = capi.fastq_read_set(ctx, text, list(range(65536, len(text), 65536 + 16)))
        assert b.tobytes() == g["r1_bases"].tobytes() and (o == g["r1_offsets"]).all()
        planes = []
        for bases, offs in ((b, o), (g["r1_bases"], g["r1_offsets"])):
            ctx.eref_set_coder(g["index_header"])
            ctx.eref_table_reset()
            db, do = ctx.upload(bases), ctx.upload(np.asarray(offs, np.int64))
            ctx.eref_count_reads(db, do, len(offs) - 1)
            pc = ctx.eref_table_popcounts()
            ptrs, nbytes = ctx.eref_table_planes()
            host = np.empty(nbytes, np.uint8)
            capi._check(capi.lib().palace_d2h(ctx.h, host.ctypes.data, ptrs[0], nbytes), "palace_d2h")
            planes.append((tuple(int(x) for x in pc), hashlib.sha256(host).hexdigest()))
            db.free(); do.free()
        assert planes[0] == planes[1] and planes[0][0][0] > 0


# ------------------------------------------------------------------------------------------------
# 2. CRC-32 of members
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_crc32_members_equals_zlib():
    rng = np.random.default_rng(3)
    lens = [0, 1, 63, 64, 65, 4095, 65536] + [int(x) for x in rng.integers(0, 65537, size=40)] + [3, 0, 7]
    data = bytes(rng.integers(0, 256, size=sum(lens), dtype=np.uint8))
    with capi.Ctx(0) as ctx:
        got = capi.crc32_members(ctx, data, lens)
    want, at = [], 0
    for L in lens:
        want.append(zlib.crc32(data[at:at + L]))
        at += L
    assert got.tolist() == want


# ------------------------------------------------------------------------------------------------
# 3-5. the executable
# ------------------------------------------------------------------------------------------------
FORMATS = ("gzip1", "gzip_multi", "bgzf4000", "bgzf_stored", "bgzf_plain", "gzip_fields")


def write_format(fmt, d, fq1, fq2):
    """(path1, path2) of the two FASTQ texts written as `fmt`"""
    out = []
    for side, text in ((1, fq1), (2, fq2)):
        p = os.path.join(d, f"{fmt}_{side}.fq.gz")
        if fmt == "gzip1":
            blob = gz.gzip_member(text, 1)
        elif fmt == "gzip_multi":                                  # members cut mid-record and mid-line
            blob = gz.gzip_members(text, [len(text) // 3 + 1, len(text) // 2 + 7, len(text) - 5], 1)
        elif fmt == "bgzf4000":                                    # records and lines straddle members
            blob = gz.bgzf(text, 4000, 1)
        elif fmt == "bgzf_stored":
            blob = gz.bgzf(text, level=0)
        elif fmt == "bgzf_plain":                                  # fq1 BGZF, fq2 plain
            if side == 2:
                p = os.path.join(d, f"{fmt}_{side}.fq")
                blob = text
            else:
                blob = gz.bgzf(text, level=1)
        else:                                                      # FEXTRA, FNAME, FCOMMENT, FHCRC, two members
            h = len(text) // 2
            blob = gz.gzip_member(text[:h], 1, fname=b"r.fq", comment=b"x", extra=b"ZZ\x01\x00q", hcrc=True) + \
                gz.gzip_member(text[h:], 1, fname=b"s")
        open(p, "wb").write(blob)
        out.append(p)
    return out


@pytest.fixture(scope="module")
def toy(golden_eref, tmp_path_factory):
    g = golden_eref
    d = str(tmp_path_factory.mktemp("eref_gz_toy"))
    fa = os.path.join(d, "db.fa")
    open(fa, "wb").write(g["db_fasta"].tobytes())
    orc.build_index_file(fa, g["index_header"], fa + ".k32.index.dat", fa + ".genome.len.txt")
    synth.ReadSet(g["r1_bases"], g["r1_offsets"]).write_fastq(os.path.join(d, "r_1.fq"), "1")
    synth.ReadSet(g["r2_bases"], g["r2_offsets"]).write_fastq(os.path.join(d, "r_2.fq"), "2")
    fq1, fq2 = (open(os.path.join(d, f"r_{s}.fq"), "rb").read() for s in (1, 2))
    files = {fmt: write_format(fmt, d, fq1, fq2) for fmt in FORMATS}
    return d, fa, files


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS)
def test_eref_compressed_toy_equals_reference_stdout(toy, golden_eref, fmt):
    d, fa, files = toy
    tmp = os.path.join(d, "tmp.txt")
    for key, hr, pr in (("stdout_090_085", "0.9", "0.85"), ("stdout_080_050", "0.8", "0.5"), ("stdout_095_090", "0.95", "0.9")):
        for threads in ("1", "8"):
            open(tmp, "w").write("stale")
            p = run([os.path.join(BIN, "eref"), *files[fmt], fa, tmp, hr, pr, threads])
            assert p.returncode == 0, p.stderr
            assert p.stdout == golden_eref[key].tobytes()
            assert os.path.getsize(tmp) == 0


@pytest.fixture(scope="module")
def cfg1_gz(tmp_path_factory):
    g = np.load(os.path.join(ROOT, "tests", "golden", "eref_50k.npz"))
    seed, n_refs, n_pairs = (int(x) for x in g["params"])
    fa_b, fq1, fq2 = synth.eref_config_inputs(seed, n_refs, n_pairs)
    assert hashlib.sha256(fq1).hexdigest() == str(g["sha256_fq1"]) and hashlib.sha256(fq2).hexdigest() == str(g["sha256_fq2"])
    d = str(tmp_path_factory.mktemp("eref_gz_50k"))
    fa = os.path.join(d, "db.fa")
    open(fa, "wb").write(fa_b)
    open(os.path.join(d, "coder.hdr"), "wb").write(g["index_header"].tobytes())
    files = {fmt: write_format(fmt, d, fq1, fq2) for fmt in ("gzip1", "gzip_multi", "bgzf4000", "bgzf_stored", "bgzf_plain")}
    return g, d, fa, files


@pytest.mark.gpu
def test_eref_compressed_50k_equals_reference_stdout(cfg1_gz):
    g, d, fa, files = cfg1_gz
    tmp = os.path.join(d, "tmp.txt")
    env = dict(os.environ, PALACE_CODER_HEADER=os.path.join(d, "coder.hdr"))   # the first run builds the index with the reference's coder
    for fmt, paths in files.items():
        for key, hr, pr, threads in (("stdout_090_085", "0.9", "0.85", "8"), ("stdout_090_085", "0.9", "0.85", "1"),
                                     ("stdout_080_050", "0.8", "0.5", "8")):
            p = run([os.path.join(BIN, "eref"), *paths, fa, tmp, hr, pr, threads], env=env)
            assert p.returncode == 0, (fmt, p.stderr)
            assert p.stdout == g[key].tobytes(), fmt
            assert os.path.getsize(tmp) == 0


@pytest.mark.gpu
def test_eref_compressed_subsampling_equals_plain(toy, golden_eref):
    """E3 on compressed input: the same draws as on the plain files (which test_gpu_cli.py pins to the oracle), also when
    hundreds of small windows carry partial lines"""
    d, fa, files = toy
    g = golden_eref
    target = str(int(g["r1_offsets"][-1]))                       # ratio 50
    hooks = os.path.join(BIN, "eref_testhooks")
    base = [fa, os.path.join(d, "t.txt"), "0.8", "0.5", "4"]
    env = dict(os.environ, PALACE_EREF_SAMPLE_TARGET=target)
    want = run([hooks, os.path.join(d, "r_1.fq"), os.path.join(d, "r_2.fq"), *base], env=env)
    assert want.returncode == 0, want.stderr
    assert want.stdout != g["stdout_080_050"].tobytes()          # sampling changes the answer
    n_text = os.path.getsize(os.path.join(d, "r_1.fq"))
    for window in (None, "4096", "208"):
        e = dict(env) if window is None else dict(env, PALACE_EREF_GZ_WINDOW=window)
        if window:
            assert n_text // int(window) >= 200                   # hundreds of windows per side
        for fmt in ("bgzf4000", "gzip_multi", "bgzf_plain"):
            p = run([hooks, *files[fmt], *base], env=e)
            assert p.returncode == 0, (fmt, window, p.stderr)
            assert p.stdout == want.stdout, (fmt, window)


@pytest.mark.gpu
def test_eref_damaged_compressed_input_fails_cleanly(toy, tmp_path):
    d, fa, files = toy
    fq1 = open(os.path.join(d, "r_1.fq"), "rb").read()
    good2 = files["bgzf4000"][1]
    cases = {}
    stored = bytearray(gz.bgzf(fq1, level=0))
    stored[18 + 5 + 1000] ^= 0x01                                 # a byte of the first member's stored data: only its CRC-32 can tell
    cases["crc.fq.gz"] = bytes(stored)
    whole = gz.gzip_member(fq1, 1)
    cases["truncated.fq.gz"] = whole[:len(whole) * 2 // 3]
    cases["garbage.fq.gz"] = whole + b"this is not gzip\n"
    cases["bgzf_garbage.fq.gz"] = gz.bgzf(fq1, 4000, 1) + b"\0\0\0\0"
    cases["bgzf_truncated.fq.gz"] = gz.bgzf(fq1, 4000, 1)[:-40]
    bad_size = bytearray(whole)
    bad_size[-1] ^= 0x10                                          # ISIZE
    cases["isize.fq.gz"] = bytes(bad_size)
    for name, blob in cases.items():
        p1 = str(tmp_path / name)
        open(p1, "wb").write(blob)
        for args in ([p1, good2], [good2, p1]):
            p = run([os.path.join(BIN, "eref"), *args, fa, str(tmp_path / "t.txt"), "0.9", "0.85", "4"])
            assert p.returncode == 1, (name, p.returncode, p.stderr)
            assert p.stdout == b"", name
            err = p.stderr.decode()
            assert p1 in err and err.count("\n") == 1, (name, err)
