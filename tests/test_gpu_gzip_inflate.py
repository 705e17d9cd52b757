"""gzip that is not BGZF, inflated on the device (palace_gzip_inflate): the text at the C ABI against zlib -- default and small
strides / spans, mixed block types, windows that reach across many chunks, several members, damaged streams -- and the eref executable
on such files against the reference's goldens, its own plain-text path and zlib's verdict on damaged files.

The counters tell the device path from the fallback: `fallback` 0 means every byte came from the device kernels."""
import hashlib
import os
import subprocess
import zlib

import numpy as np
import pytest

from palace_amd import capi, synth
from tests import gz_util as gz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "palace_amd", "bin")
LEVELS = (1, 6, 9)
# DEFLATE blocks of the 50k FASTQ files (52 MB of text each), counted on the CPU with zlib's Z_BLOCK (`bin/gzip_selftest blocks`):
#   level 1: 9.94 MB, 402 blocks (401 dynamic and not final) -- one every 24.7 KB of compressed data
#   level 6: 8.71 MB, 301 blocks (300)                        -- one every 28.9 KB
#   level 9: 8.59 MB, 285 blocks (284)                        -- one every 30.1 KB
# The default stride of 16 KiB is below that spacing, so nearly every block start is the first one of some stride; where two starts
# fall into one stride the second is not looked for and its block rides with the one before it.


def run(cmd, **kw):
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, **kw)


@pytest.fixture(scope="module")
def texts(golden_eref, tmp_path_factory):
    """(toy FASTQ side 1, 50k FASTQ side 1, 50k FASTQ side 2, 50k FASTA)"""
    g = golden_eref
    d = str(tmp_path_factory.mktemp("gz_texts"))
    synth.ReadSet(g["r1_bases"], g["r1_offsets"]).write_fastq(os.path.join(d, "r_1.fq"), "1")
    toy = open(os.path.join(d, "r_1.fq"), "rb").read()
    k = np.load(os.path.join(ROOT, "tests", "golden", "eref_50k.npz"))
    seed, n_refs, n_pairs = (int(x) for x in k["params"])
    fa, fq1, fq2 = synth.eref_config_inputs(seed, n_refs, n_pairs)
    assert hashlib.sha256(fq1).hexdigest() == str(k["sha256_fq1"])
    return toy, fq1, fq2, fa


def check(ctx, blob, want, **kw):
    """the device path's text == want, no fallback, no guard byte touched; returns the counters"""
    text, st = capi.gzip_inflate(ctx, blob, check_guards=True, **kw)
    print({k: v for k, v in st.items() if not k.startswith("ms_")}, kw)
    assert st["guards_bad"] == 0
    assert st["fallback"] == 0, st
    assert text is not None and len(text) == len(want) and text == want
    assert st["text_bytes"] == len(want)
    return st


# ------------------------------------------------------------------------------------------------
# at the C ABI, against zlib
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gzip_levels_equal_zlib(texts):
    toy, fq1, fq2, _ = texts
    with capi.Ctx(0) as ctx:
        for level in LEVELS:
            blob = gz.gzip_member(toy, level)
            check(ctx, blob, zlib.decompress(blob, 31))
            for fq in (fq1, fq2):
                blob = gz.gzip_member(fq, level)
                st = check(ctx, blob, zlib.decompress(blob, 31))
                assert st["chunks_accepted"] > 1 and st["members"] == 1


@pytest.mark.gpu
def test_gzip_small_stride_and_span_and_one_chunk(texts):
    _, fq1, _, _ = texts
    with capi.Ctx(0) as ctx:
        for level in LEVELS:
            blob = gz.gzip_member(fq1, level)
            want = zlib.decompress(blob, 31)
            st = check(ctx, blob, want, stride=1024, span=len(blob) // 5 + 1)
            assert st["chunks_accepted"] >= 200 and st["spans"] >= 5                   # hundreds of chunks, several spans
            st = check(ctx, blob, want, stride=1024, span=len(blob) // 5 + 1, text_cap=1 << 20)   # ... and several batches per span
            assert st["batches"] > st["spans"]
            if level == 6:                                                             # one wavefront decodes the whole file
                st = check(ctx, blob, want, stride=len(blob) + 1000)
                assert st["chunks_accepted"] == 1 and st["chunks_found"] == 0


@pytest.mark.gpu
def test_gzip_mixed_block_types(texts):
    _, fq1, _, _ = texts
    rng = np.random.default_rng(17)
    with capi.Ctx(0) as ctx:
        # Z_FULL_FLUSH every 300 KB: empty stored blocks and a window reset in the middle of the stream
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        parts = []
        for at in range(0, len(fq1), 300_000):
            parts.append(c.compress(fq1[at:at + 300_000]))
            parts.append(c.flush(zlib.Z_FULL_FLUSH))
        blob = b"".join(parts) + c.flush()
        assert zlib.decompress(blob, 31) == fq1
        check(ctx, blob, fq1)
        check(ctx, blob, fq1, stride=2048, span=200_000)
        # text and random bytes in turns: stored blocks of data between dynamic ones
        mixed = b"".join(fq1[i * 200_000:(i + 1) * 200_000] + bytes(rng.integers(0, 256, size=70_000, dtype=np.uint8)) for i in range(12))
        blob = gz.gzip_member(mixed, 6)
        check(ctx, blob, mixed)
        check(ctx, blob, mixed, stride=4096, span=300_000)
        # level 0: stored blocks only; the finder looks for none of them, one wavefront decodes the file
        blob = gz.gzip_member(fq1[:500_000], 0)
        st = check(ctx, blob, fq1[:500_000])
        assert st["chunks_found"] == 0 and st["chunks_accepted"] == 1


@pytest.mark.gpu
def test_gzip_windows_reach_across_many_chunks(texts):
    _, _, _, fa = texts
    rng = np.random.default_rng(23)
    with capi.Ctx(0) as ctx:
        fa = fa[:20_000_000]
        blob = gz.gzip_member(fa, 6)
        st = check(ctx, blob, fa, stride=2048)
        assert st["chunks_accepted"] > 1
        # a period of 32 700 bytes, half of it fresh text and half of it the same 16 350 bytes every time: those are matches that
        # reach almost a whole window back, so their bytes are known only through a chain of references that crosses every chunk
        # before them, while the fresh halves keep the blocks coming
        acgt = np.frombuffer(b"ACGT", np.uint8)
        same = bytes(rng.choice(acgt, size=16_350))
        rep = b"".join(bytes(rng.choice(acgt, size=16_350)) + same for _ in range(200))
        for level in (1, 9):
            blob = gz.gzip_member(rep, level)
            st = check(ctx, blob, rep, stride=512)
            assert st["chunks_accepted"] > 10
        # structured binary records
        recs = np.zeros((200_000, 4), np.uint32)
        recs[:, 0] = np.arange(200_000)
        recs[:, 1] = rng.integers(0, 50, size=200_000)
        recs[:, 3] = 0xDEADBEEF
        blob = gz.gzip_member(recs.tobytes(), 6)
        st = check(ctx, blob, recs.tobytes(), stride=4096)
        assert st["chunks_accepted"] > 1


@pytest.mark.gpu
def test_gzip_members_and_header_fields(texts):
    """several members take the device path too: the member behind a trailer is a certain start the chain queues"""
    toy, fq1, _, _ = texts
    with capi.Ctx(0) as ctx:
        for text in (toy, fq1):
            blob = gz.gzip_members(text, [len(text) // 3 + 1, len(text) // 2 + 7, len(text) - 5], 1)
            st = check(ctx, blob, text)
            assert st["members"] == 4                             # (a member that opens with a dynamic block is also a finder hit)
            check(ctx, blob, text, stride=1024, span=len(blob) // 3 + 1)
            blob = gz.gzip_member(text, 6, fname=b"r_1.fq", comment=b"a comment", extra=b"XY\x02\x00ab", hcrc=True)
            st = check(ctx, blob, text)
            assert st["members"] == 1
            h = len(text) // 2
            blob = gz.gzip_member(text[:h], 1, fname=b"r.fq", comment=b"x", extra=b"ZZ\x01\x00q", hcrc=True) + gz.gzip_member(text[h:], 1, fname=b"s")
            assert check(ctx, blob, text)["members"] == 2
        blob = gz.gzip_member(b"", 6) + gz.gzip_member(b"@a\nACGT\n+\nIIII\n", 6) + gz.gzip_member(b"", 6)
        assert check(ctx, blob, b"@a\nACGT\n+\nIIII\n")["members"] == 3
        # more members in one span than the chain queues: declined, and the counter says why
        many = gz.gzip_members(toy, list(range(1000, 40_000, 1000)), 1)
        text, st = capi.gzip_inflate(ctx, many, check_guards=True)
        print(st)
        assert st["guards_bad"] == 0 and (st["fallback"] == 3 and text is None or text == toy)


def zlib_verdict(blob):
    """(text or None) of a whole gzip file as zlib reads it: every member, nothing but members"""
    out, rest = [], blob
    try:
        while rest:
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
            if not d.eof:
                return None
            rest = d.unused_data
    except zlib.error:
        return None
    return b"".join(out)


@pytest.mark.gpu
def test_gzip_damaged_streams_never_give_wrong_text(texts):
    """Runs once.  The output buffers of every batch lie between guard bytes that the call checks (guards_bad)."""
    _, fq1, _, _ = texts
    good = gz.gzip_member(fq1, 6)
    n = len(good)
    cases = {}
    for name, at in (("bit flip mid-stream", n // 2), ("bit flip in the first block header", 10 + 3), ("bit flip later", n * 3 // 4 + 11)):
        b = bytearray(good)
        b[at] ^= 0x10
        cases[name] = bytes(b)
    with capi.Ctx(0) as ctx:
        _, st0 = capi.gzip_inflate(ctx, good)
        assert st0["fallback"] == 0
        cases["truncated at two thirds"] = good[:n * 2 // 3]
        b = bytearray(good); b[-8] ^= 0x01
        cases["wrong CRC"] = bytes(b)
        b = bytearray(good); b[-1] ^= 0x10
        cases["wrong ISIZE"] = bytes(b)
        cases["garbage behind the member"] = good + b"this is not gzip\n"
        for at in range(n // 3, n // 3 + 24):                     # ... and flips of which nothing is assumed: whatever they hit
            b = bytearray(good)                                   # (a literal, a length, a header), the rule below holds
            b[at] ^= 1 << (at & 7)
            cases[f"bit flip at byte {at}"] = bytes(b)
        for name, blob in cases.items():
            want = zlib_verdict(blob)
            for kw in ({}, {"stride": 2048, "span": n // 4}):
                text, st = capi.gzip_inflate(ctx, blob, check_guards=True, **kw)
                print(name, kw, "zlib:", "ok" if want is not None else "error", "fallback", st["fallback"])
                assert st["guards_bad"] == 0, name
                if st["fallback"] == 0:
                    assert want is not None and text == want, name        # a success is an exact result
                else:
                    assert text is None
                if want is None:
                    assert st["fallback"] != 0, name
        assert capi.gzip_inflate(ctx, b"plain text\n")[1]["fallback"] == 1
        assert capi.gzip_inflate(ctx, b"")[1]["fallback"] == 1


# ------------------------------------------------------------------------------------------------
# through the executable
# ------------------------------------------------------------------------------------------------
def device_lines(stderr):
    return [ln for ln in stderr.decode().splitlines() if ln.startswith("[eref] gzip on the device: ")]


@pytest.fixture(scope="module")
def toy_dir(golden_eref, tmp_path_factory):
    from oracle import binding as orc
    g = golden_eref
    d = str(tmp_path_factory.mktemp("gz_toy"))
    fa = os.path.join(d, "db.fa")
    open(fa, "wb").write(g["db_fasta"].tobytes())
    orc.build_index_file(fa, g["index_header"], fa + ".k32.index.dat", fa + ".genome.len.txt")
    synth.ReadSet(g["r1_bases"], g["r1_offsets"]).write_fastq(os.path.join(d, "r_1.fq"), "1")
    synth.ReadSet(g["r2_bases"], g["r2_offsets"]).write_fastq(os.path.join(d, "r_2.fq"), "2")
    fq = [open(os.path.join(d, f"r_{s}.fq"), "rb").read() for s in (1, 2)]
    for level in LEVELS:
        for s in (1, 2):
            open(os.path.join(d, f"l{level}_{s}.fq.gz"), "wb").write(gz.gzip_member(fq[s - 1], level))
    return d, fa, fq


@pytest.mark.gpu
def test_eref_gzip_toy_equals_reference_stdout(toy_dir, golden_eref):
    d, fa, _ = toy_dir
    tmp = os.path.join(d, "tmp.txt")
    for level in LEVELS:
        files = [os.path.join(d, f"l{level}_{s}.fq.gz") for s in (1, 2)]
        for key, hr, pr in (("stdout_090_085", "0.9", "0.85"), ("stdout_080_050", "0.8", "0.5")):
            p = run([os.path.join(BIN, "eref"), *files, fa, tmp, hr, pr, "4"])
            assert p.returncode == 0, p.stderr
            assert p.stdout == golden_eref[key].tobytes()
            assert p.stderr == b""
        p = run([os.path.join(BIN, "eref"), *files, fa, tmp, "0.9", "0.85", "4"], env=dict(os.environ, PALACE_TRACE="1"))
        assert p.returncode == 0 and p.stdout == golden_eref["stdout_090_085"].tobytes()
        lines = device_lines(p.stderr)
        assert len(lines) == 2 and all("device path" in ln and "fallback 0;" in ln for ln in lines), lines


@pytest.mark.gpu
def test_eref_gzip_50k_equals_reference_stdout_on_the_device_path(tmp_path):
    g = np.load(os.path.join(ROOT, "tests", "golden", "eref_50k.npz"))
    seed, n_refs, n_pairs = (int(x) for x in g["params"])
    fa_b, fq1, fq2 = synth.eref_config_inputs(seed, n_refs, n_pairs)
    fa = str(tmp_path / "db.fa")
    open(fa, "wb").write(fa_b)
    open(str(tmp_path / "coder.hdr"), "wb").write(g["index_header"].tobytes())
    env = dict(os.environ, PALACE_CODER_HEADER=str(tmp_path / "coder.hdr"), PALACE_TRACE="1")
    tmp = str(tmp_path / "tmp.txt")
    for level in LEVELS:
        files = []
        for s, text in ((1, fq1), (2, fq2)):
            files.append(str(tmp_path / f"l{level}_{s}.fq.gz"))
            open(files[-1], "wb").write(gz.gzip_member(text, level))
        for key, hr, pr in (("stdout_090_085", "0.9", "0.85"), ("stdout_080_050", "0.8", "0.5")):
            p = run([os.path.join(BIN, "eref"), *files, fa, tmp, hr, pr, "8"], env=env)
            assert p.returncode == 0, p.stderr
            assert p.stdout == g[key].tobytes(), level
            lines = device_lines(p.stderr)
            assert len(lines) == 2, p.stderr
            for ln in lines:
                assert "device path" in ln and "fallback 0;" in ln, ln
                assert int(ln.split("accepted ")[1].split(",")[0]) > 1, ln


@pytest.mark.gpu
def test_eref_gzip_subsampling_equals_plain(toy_dir, golden_eref):
    d, fa, _ = toy_dir
    g = golden_eref
    hooks = os.path.join(BIN, "eref_testhooks")
    base = [fa, os.path.join(d, "t.txt"), "0.8", "0.5", "4"]
    env = dict(os.environ, PALACE_EREF_SAMPLE_TARGET=str(int(g["r1_offsets"][-1])), PALACE_TRACE="1")
    want = run([hooks, os.path.join(d, "r_1.fq"), os.path.join(d, "r_2.fq"), *base], env=env)
    assert want.returncode == 0, want.stderr
    assert want.stdout != g["stdout_080_050"].tobytes()
    files = [os.path.join(d, f"l6_{s}.fq.gz") for s in (1, 2)]
    # (a span has to hold a whole block, tens of KB here: a smaller one is declined as "no progress" and zlib reads the file)
    for extra in ({}, {"PALACE_EREF_GZ_STRIDE": "512", "PALACE_EREF_GZ_SPAN": "120000", "PALACE_EREF_GZ_WINDOW": "4096"}):
        p = run([hooks, *files, *base], env=dict(env, **extra))
        assert p.returncode == 0, p.stderr
        assert p.stdout == want.stdout, extra
        lines = device_lines(p.stderr)
        assert len(lines) == 2 and all("fallback 0;" in ln for ln in lines), lines
        if extra:
            assert all(int(ln.split("spans ")[1].split(",")[0]) > 1 for ln in lines), lines


@pytest.mark.gpu
def test_eref_damaged_gzip_fails_cleanly(toy_dir, tmp_path):
    d, fa, fq = toy_dir
    whole = gz.gzip_member(fq[0], 1)
    good2 = os.path.join(d, "l1_2.fq.gz")
    cases = {"truncated.fq.gz": whole[:len(whole) * 2 // 3], "garbage.fq.gz": whole + b"this is not gzip\n"}
    b = bytearray(whole); b[-1] ^= 0x10
    cases["isize.fq.gz"] = bytes(b)
    # a bit flip in the middle of the stream that only the CRC can tell: the first one zlib reads to the end
    for at in range(len(whole) // 2, len(whole) - 8):
        b = bytearray(whole); b[at] ^= 0x04
        try:
            zlib.decompress(bytes(b), 31)
        except zlib.error as e:
            if "incorrect data check" in str(e):
                cases["crc_only.fq.gz"] = bytes(b)
                break
    assert "crc_only.fq.gz" in cases
    for name, blob in cases.items():
        p1 = str(tmp_path / name)
        open(p1, "wb").write(blob)
        for args in ([p1, good2], [good2, p1]):
            p = run([os.path.join(BIN, "eref"), *args, fa, str(tmp_path / "t.txt"), "0.9", "0.85", "4"])
            assert p.returncode == 1, (name, p.returncode, p.stderr)
            assert p.stdout == b"", name
            err = p.stderr.decode()
            assert p1 in err and err.count("\n") == 1, (name, err)


def block_starts(path):
    """[(bit of the file, BTYPE, BFINAL)] of a gzip file, from zlib on the CPU"""
    out = run([os.path.join(BIN, "gzip_selftest"), "blocks", path])
    assert out.returncode == 0, out.stderr
    return [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().splitlines()[:-1]]


@pytest.mark.gpu
def test_gzip_span_that_ends_inside_a_block_header(texts, tmp_path):
    """A span's last chunk meets a block header that the span cuts off: that says "more input" (the next span starts at that block),
    not "bad code" -- the file stays on the device path."""
    _, fq1, _, _ = texts
    blob = gz.gzip_member(fq1, 6)
    path = str(tmp_path / "f.gz")
    open(path, "wb").write(blob)
    starts = block_starts(path)
    assert len(starts) == 301 and sum(1 for _, t, f in starts if t == 2 and not f) == 300
    with capi.Ctx(0) as ctx:
        for k in (3, 100, 299):
            bit, btype, bfinal = starts[k]
            assert btype == 2
            for into in (0, 1, 2, 9, 20, 45, 70):                      # bytes of the header inside the span (a header is ~80 bytes here)
                span = (bit >> 3) + 1 + into - 8                        # the first span starts at byte 8 (the DEFLATE data at byte 10)
                st = check(ctx, blob, fq1, span=span)
                assert st["spans"] >= 2, (k, into, st)


@pytest.mark.gpu
def test_eref_good_file_declined_after_part_of_it_was_parsed(toy_dir, golden_eref):
    """One large member, then 40 small ones: with small spans the first spans are parsed on the device, a later one has more member
    starts than the chain queues, the file is declined, its reads are taken back and zlib reads it again -- stdout as on plain text."""
    d, fa, fq = toy_dir
    hooks = os.path.join(BIN, "eref_testhooks")
    base = [fa, os.path.join(d, "t.txt"), "0.8", "0.5", "4"]
    want = run([hooks, os.path.join(d, "r_1.fq"), os.path.join(d, "r_2.fq"), *base])
    assert want.returncode == 0 and want.stdout == golden_eref["stdout_080_050"].tobytes()
    files = []
    for s in (1, 2):
        text = fq[s - 1]
        h = len(text) * 3 // 4
        cuts = [h + 200 * i for i in range(1, 40)]
        blob = gz.gzip_member(text[:h], 6) + gz.gzip_members(text[h:], [c - h for c in cuts], 1)
        assert zlib_verdict(blob) == text
        files.append(os.path.join(d, f"declined_{s}.fq.gz"))
        open(files[-1], "wb").write(blob)
    env = dict(os.environ, PALACE_TRACE="1", PALACE_EREF_GZ_SPAN="120000", PALACE_EREF_GZ_WINDOW="4096")
    for args in (files, [files[0], os.path.join(d, "r_2.fq")], [os.path.join(d, "l6_1.fq.gz"), files[1]]):
        p = run([hooks, *args, *base], env=env)
        assert p.returncode == 0, p.stderr
        assert p.stdout == want.stdout
        lines = [ln for ln in device_lines(p.stderr) if "declined_" in ln]
        assert lines and all("declined, zlib" in ln and "fallback 3;" in ln for ln in lines), lines
        assert all(int(ln.split("spans ")[1].split(",")[0]) > 1 for ln in lines), lines    # earlier spans had been parsed
