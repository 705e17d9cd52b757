"""The rules of `samview` on a CPU: the Python restatement of tests/sam_cases.py against the byte-by-byte BAM encoder
of tests/test_host_bam_spec.py (written against the specification, independently of both); csrc/sam_line.hpp and
host/sam_header.hpp -- driven by the stand-alone `sam_line_selftest`, as built and under ASan + UBSan -- against the restatement;
the borders of the integer tags, QNAME, the op count and POS; and `samview` / `bamsort --sam` where no device is visible or the
command line is wrong.  (The kernels: tests/test_gpu_sam_encode.py; the tools on a device: tests/test_gpu_samview_cli.py.)"""
import os
import struct
import subprocess

import pytest

from palace_amd import capi
from tests import sam_cases as sc
from tests.test_host_bam_spec import aux_A, aux_B, aux_C, aux_H, aux_Z, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
TOOLS = [os.path.join(BIN, t) for t in ("sam_line_selftest", "sam_line_selftest_asan")]
SEED = 7                                             # (chosen so that the restatement alone meets test_generated_lines' conditions)


@pytest.fixture(scope="module", autouse=True)
def built():
    capi.build()
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in ("sam_line_selftest", "sam_line_selftest_asan", "samview", "bamsort")],
                   check=True, stdout=subprocess.DEVNULL)


# ---- the restatement against the specification's encoder -----------------------------------------------------------------------------
NIBBLE = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}          # SAM specification 4.2: the 4-bit base codes


def spec_record(qname, flag, tid, pos, mapq, cigar, mtid, mpos, tlen, seq, qual, bin_, aux=b""):
    """record(...) of test_host_bam_spec.py, which writes bin 4680, tlen 0, bases A and qualities 40, with those four put right:
    seq = the bases as text, qual = the stored values (None: 0xff each), bin_ = the bin worked out by hand"""
    raw = bytearray(record(qname, flag, tid, pos, mapq, cigar, mtid=mtid, mpos=mpos, l_seq=len(seq), aux=aux))
    n_ops = struct.unpack_from("<H", raw, 4 + 12)[0]
    struct.pack_into("<H", raw, 4 + 10, bin_)
    struct.pack_into("<i", raw, 4 + 28, tlen)
    at = 4 + 32 + len(qname) + 1 + 4 * n_ops
    nib = [NIBBLE.get(c.upper(), 15) for c in seq] + [0]
    for j in range((len(seq) + 1) // 2):
        raw[at + j] = nib[2 * j] << 4 | nib[2 * j + 1]
    at += (len(seq) + 1) // 2
    raw[at:at + len(seq)] = bytes(qual) if qual is not None else b"\xff" * len(seq)
    return bytes(raw)


SA1, SA2 = "ref,29,-,6H5M,17,0;", "ref,9,+,5S6M,30,1;"
TAGS_AUX = (aux_A("XA", "!") + aux_H("XH", "") + aux_H("Xh", "1aF0") + aux_Z("XZ", "") + aux_B("Zc", "c", []) + aux_B("ZC", "C", [0, 255]) +
            aux_B("Zs", "s", [-32768, 32767]) + aux_B("ZS", "S", [65535]) + aux_B("Zi", "i", [-2**31, 2**31 - 1]) + aux_B("ZI", "I", [4294967295]) +
            aux_C("Xi", 0) + aux_C("X0", 7))
SPEC_CASES = [          # (line, the record by the specification's encoder)
    (sc.SPEC_READS[0], spec_record("r001", 99, 0, 6, 30, "8M2I4M1D3M", 0, 36, 39, "TTAGATAAAGGATACTG", None, 4681)),
    (sc.SPEC_READS[1], spec_record("r002", 0, 0, 8, 30, "3S6M1P1I4M", -1, -1, 0, "AAAAGATAAGGATA", None, 4681)),
    (sc.SPEC_READS[2], spec_record("r003", 0, 0, 8, 30, "5S6M", -1, -1, 0, "GCCTAAGCTAA", None, 4681, aux_Z("SA", SA1))),
    (sc.SPEC_READS[3], spec_record("r004", 0, 0, 15, 30, "6M14N5M", -1, -1, 0, "ATAGCTTCAGC", None, 4681)),
    (sc.SPEC_READS[4], spec_record("r003", 2064, 0, 28, 17, "6H5M", -1, -1, 0, "TAGGC", None, 4681, aux_Z("SA", SA2))),
    (sc.SPEC_READS[5], spec_record("r001", 147, 0, 36, 30, "9M", 0, 6, -39, "CAGCGGCAT", None, 4681, aux_C("NM", 1))),
    (sc.HAND_VALID[6], spec_record("pair/1", 73, 0, 11, 60, "5M", 0, 11, 0, "ACGTN", [40, 40, 40, 40, 2], 4681,
                                   aux_C("NM", 0) + b"ASc" + struct.pack("<b", -5) + b"XSS" + struct.pack("<H", 300) + aux_Z("MD", "5"))),
    # an unmapped mate that carries RNAME / POS: it keeps them, and is filed under one base
    (sc.HAND_VALID[7], spec_record("pair/2", 133, 0, 11, 0, [], 0, 11, 0, "acgtn", [0, 0, 93, 93, 20], 4681)),
    # an RNAME with POS 0 is no place; RNEXT by name stays
    (sc.HAND_VALID[8], spec_record("zero", 0, -1, -1, 0, "4M", 1, 4, -2**31, "ACGT", None, 4680)),
    # ... and RNEXT '=' is the refID as encoded
    (b"zeq\t0\tref\t0\t0\t4M\t=\t5\t0\tACGT\t*", spec_record("zeq", 0, -1, -1, 0, "4M", -1, 4, 0, "ACGT", None, 4680)),
    # no CIGAR on a record whose flag says mapped: 0x4 is set; bin = (4681 + (pos >> 14)) mod 2^16 at the largest POS
    (sc.HAND_VALID[9], spec_record("nocig", 4, 2, 2147483646, 255, [], -1, -1, 2147483647, "", None, (4681 + 131071) & 0xffff)),
    (sc.HAND_VALID[10], spec_record("tags", 4, -1, -1, 0, [], -1, -1, 0, "RYKMSWBDHVN=.x", None, 4680, TAGS_AUX)),
    # [16383, 16386) crosses a 16 kb border: level 4, bin 585
    (sc.HAND_VALID[12], spec_record("odd", 0, 1, 16383, 7, "3M", 1, 0, -16383, "TGA", [32, 33, 34], 585)),
]


def test_restatement_against_the_specifications_encoder():
    for line, want in SPEC_CASES:
        assert sc.encode(line, sc.NAMES) == want, line
    assert SPEC_CASES[12][1][4 + 32 + 4 + 4:][:2] == b"\x84\x10"                          # TGA: high nibble first, the odd one's low nibble 0
    assert sc.encode(sc.HAND_VALID[11], sc.NAMES)[4 + 12:4 + 14] == struct.pack("<H", 9)  # all nine ops
    for line, code in sc.HAND_ERRORS:
        assert sc.encode(line, sc.NAMES) == code, line
    assert sc.encode(sc.SPEC_READS[4], sc.NAMES, 0x800) is sc.DROPPED and isinstance(sc.encode(sc.SPEC_READS[4], sc.NAMES, 0x7ef), bytes)
    assert sc.encode(b"a\t2048\tnone\t1\t0\t1M\t*\t0\t0\tA\t*", sc.NAMES, 0x800) == sc.ERNAME   # a malformed dropped line is still an error


def test_restatement_of_the_header():
    head, n_head, targets = sc.header_of(sc.HEADER + sc.SPEC_READS[0] + b"\n")
    assert (head, n_head, targets) == (sc.HEADER, 5, sc.TARGETS)
    assert sc.bam_header(sc.HEADER)[:8] == b"BAM\1" + struct.pack("<i", len(sc.HEADER)) and sc.bam_header(b"")[4:] == bytes(8)
    assert sc.header_of(b"@HD\tVN:1.6") == (b"@HD\tVN:1.6", 1, []) and sc.header_of(b"r\t0\n@SQ\tSN:a\tLN:1\n") == (b"", 0, [])
    for text, want in ((b"@SQ\tLN:5\n", (sc.EHDSQ, 1)), (b"@HD\n@SQ\tSN:a\n", (sc.EHDSQ, 2)), (b"@SQ\tSN:a\tLN:0\n", (sc.EHDSQ, 1)), (b"@SQ\tSN:\tLN:4\n", (sc.EHDSQ, 1)),
                       (b"@SQ\tSN:a\tLN:2147483648\n", (sc.EHDSQ, 1)), (b"@SQ\tSN:a\tLN:0x10\n", (sc.EHDSQ, 1)), (b"@SQ\tSN:a\tLN:4\n@CO\tx\n@SQ\tLN:9\tSN:a", (sc.EHDDUP, 3))):
        assert sc.header_of(text) == want, text
    assert sc.lines_verdict(b"@HD\na\n\nb") == (1, 3, 3, sc.EEMPTY) and sc.lines_verdict(b"@HD\na\n@CO\n\n") == (1, 3, 3, sc.EAT)
    assert sc.lines_verdict(b"") == (0, 0, 0, 0) and sc.lines_verdict(b"\n") == (0, 1, 1, sc.EEMPTY) and sc.lines_verdict(b"a\r\n") == (0, 1, 0, 0)


# ---- sam_line.hpp and sam_header.hpp against the restatement ---------------------------------------------------------------------------
def dump(tool, tmp_path, text, mask=0):
    path = tmp_path / "in.sam"
    path.write_bytes(text)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([tool, str(path), "%#x" % mask], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", p.stderr[-2000:]
    return p.stdout.split(b"\n")[:-1]


def expected(text, mask=0):
    head = sc.header_of(text)
    if isinstance(head[0], int):
        return [b"H %d" % head[0]]
    names, out = [n for n, _ in head[2]], []
    for line in sc.split_lines(text)[head[1]:]:
        r = sc.EEMPTY if line == b"" else sc.EAT if line.startswith(b"@") else sc.encode(line, names, mask)
        out.append(b"E %d" % r if isinstance(r, int) else b"D" if r is sc.DROPPED else b"R " + r.hex().encode())
    return out


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_hand_cases(tool, tmp_path):
    lines = sc.HAND_VALID + [l for l, _ in sc.HAND_ERRORS] + [l for l, _ in SPEC_CASES]
    for mask in (0, 0x800, 0xffff):
        for text in (sc.HEADER + b"\n".join(lines) + b"\n", sc.HEADER + b"\n".join(lines)):
            assert dump(tool, tmp_path, text, mask) == expected(text, mask)
    got = dump(tool, tmp_path, sc.HEADER + b"\n".join(l for l, _ in SPEC_CASES))
    assert got == [b"R " + r.hex().encode() for _, r in SPEC_CASES]          # ... and straight against the specification's encoder
    for text in (b"", b"\n", b"@HD\tVN:1.6", b"@SQ\tLN:5\n", b"@SQ\tSN:a\tLN:4\n@CO\tx\n@SQ\tLN:9\tSN:a", b"@SQ\tSN:a\tLN:2147483648\nr\t0\ta\n",
                 b"r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*", b"@CO\n\n@CO\nr\n"):
        assert dump(tool, tmp_path, text) == expected(text), text
    assert expected(b"@SQ\tLN:5\n") == [b"H %d" % sc.EHDSQ] and expected(b"@CO\n\n@CO\nr\n") == [b"E 2", b"E 1", b"E 3"]


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_generated_lines(tool, tmp_path):
    lines = sc.generated(SEED, 2000)
    text = sc.HEADER + b"\n".join(lines) + b"\n"
    want = expected(text)
    assert len(want) == 2000 and sum(1 for w in want if w.startswith(b"R")) >= 1000
    assert {int(w[2:]) for w in want if w.startswith(b"E")} == sc.LINE_CODES                # every code a line can have occurs
    assert dump(tool, tmp_path, text) == want
    want = expected(text, 0x800)
    assert sum(1 for w in want if w == b"D") > 100
    assert dump(tool, tmp_path, text, 0x800) == want


def field_line(**kw):
    f = dict(qname=b"q", flag=b"0", rname=b"ref", pos=b"1", mapq=b"0", cigar=b"1M", rnext=b"*", pnext=b"0", tlen=b"0", seq=b"A", qual=b"*", tags=[])
    f.update(kw)
    return b"\t".join([f[k] for k in ("qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual")] + f["tags"])


@pytest.mark.parametrize("tool", TOOLS, ids=["plain", "asan"])
def test_borders(tool, tmp_path):
    lines, want = [], []
    for v, t in sc.INT_BORDERS:                      # the smallest type that holds the value, by its sign
        lines.append(field_line(tags=[b"XX:i:%d" % v]))
        want.append(b"E %d" % t if isinstance(t, int) else t)
    lines += [field_line(qname=b"n" * 254), field_line(qname=b"n" * 255), field_line(cigar=b"1M" * 65535, seq=b"*"), field_line(cigar=b"1M" * 65536, seq=b"*"),
              field_line(pos=b"2147483647"), field_line(pos=b"2147483648"), field_line(pnext=b"2147483647"), field_line(pnext=b"2147483648")]
    text = sc.HEADER + b"\n".join(lines) + b"\n"
    got = dump(tool, tmp_path, text)
    assert got == expected(text)
    tail = 4 + 32 + 2 + 4 + 1 + 1                    # block_size, fixed part, "q\0", one op, one base, one quality
    fmt = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
    for (v, t), g in zip(sc.INT_BORDERS, got):
        if isinstance(t, int):
            assert g == b"E %d" % t
        else:
            aux = bytes.fromhex(g[2:].decode())[tail:]
            assert aux[:3] == b"XX" + t and struct.unpack(fmt[t], aux[3:])[0] == v, (v, g)
    rest = got[len(sc.INT_BORDERS):]
    assert [r[:1] for r in rest] == [b"R", b"E", b"R", b"E", b"R", b"E", b"R", b"E"]
    assert rest[1::2] == [b"E %d" % c for c in (sc.EQNAME, sc.ECIGAR, sc.EPOS, sc.EPNEXT)]
    r254, r_ops, r_pos = (bytes.fromhex(r[2:].decode()) for r in rest[0:5:2])
    assert r254[4 + 8] == 255 and r254[4 + 32:4 + 32 + 255] == b"n" * 254 + b"\0"
    assert struct.unpack_from("<H", r_ops, 4 + 12)[0] == 65535 and len(r_ops) == 4 + 32 + 2 + 4 * 65535
    assert struct.unpack_from("<i", r_pos, 4 + 4)[0] == 2147483646


# ---- the tools without a device, or with a wrong command line ----------------------------------------------------------------------------
def run(tool, args, env=None, stdin=b""):
    return subprocess.run([os.path.join(BIN, tool)] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def test_samview_without_a_device_or_with_a_wrong_command_line(tmp_path):
    sam = tmp_path / "in.sam"
    sam.write_bytes(sc.HEADER + sc.SPEC_READS[0] + b"\n")
    out = str(tmp_path / "out.bam")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    for args, stdin in ((["-@", "4", "-F", "0x0800", "-buS", "-"], sam.read_bytes()), (["-b", "-o", out, str(sam)], b""), (["-bSho" + out, "-F2048", "-@2", str(sam)], b"")):
        p = run("samview", args, env, stdin)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.startswith(b"samview:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1, p.stderr
    for args in ([], ["-b"], ["-b", str(sam), str(sam)], ["-b", "-F"], ["-b", "-F", "0x", str(sam)], ["-b", "-F", "010x", str(sam)], ["-b", "-F", "65536", str(sam)],
                 ["-b", "-F", "-1", str(sam)], ["-b", "-@", "x", str(sam)], ["-b", "-o"], ["-bq", str(sam)], ["-b", "--threads", "4", str(sam)], ["-b1", str(sam)],
                 ["-b", "-f", "4", str(sam)], ["-C", str(sam)]):
        p = run("samview", args, env)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"Usage: samview") and b"unpinned" in p.stderr and b"type f" in p.stderr, args
    for args in (["-S", str(sam)], ["-h", "-@", "2", "-o", out, str(sam)], ["-uS", "-"]):
        p = run("samview", args, env)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"samview: only BAM is written") and p.stderr.count(b"\n") == 1, args
    assert os.listdir(tmp_path) == ["in.sam"]


def test_bamsort_sam_without_a_device_or_with_a_wrong_command_line(tmp_path):
    sam = tmp_path / "in.sam"
    sam.write_bytes(sc.HEADER + sc.SPEC_READS[0] + b"\n")
    out = str(tmp_path / "out.bam")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    for args, stdin in ((["--sam", "-F", "0x0800", "-@", "4", "-", "-O", "BAM", "-o", out, "--bai"], sam.read_bytes()), (["--sam", "-o", out, str(sam)], b""),
                        (["-F2048", "-o" + out, str(sam), "--sam"], b"")):
        p = run("bamsort", args, env, stdin)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.startswith(b"bamsort:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1, p.stderr
    for args in (["--sam", "-o", out], ["--sam", "-F", "-o", out, str(sam)], ["--sam", "-F", "0y1", "-o", out, str(sam)], ["-F", "4", "-o", out, str(sam)], ["-o", out, "-"],
                 ["--sam", "-o", out, "-", "-"], ["--sam", "--index", str(sam)], ["--sam", "-u", "-o", out, str(sam)]):
        p = run("bamsort", args, env)
        assert p.returncode == 1 and p.stdout == b"" and b"Usage: bamsort" in p.stderr and b"--sam [-F <mask>]" in p.stderr, args
    assert os.listdir(tmp_path) == ["in.sam"]


def test_the_abi_declares_the_entry_points():
    names = {"palace_sam_scratch_bytes", "palace_sam_lines", "palace_sam_plan", "palace_sam_encode"}
    assert names <= set(capi.declared_symbols()) and names <= set(capi._SIGS)
    text = open(os.path.join(ROOT, "include", "palace_hip.h")).read()
    assert f"#define PALACE_SAM_TILE {capi.SAM_TILE} " in text
    for name in ("EAT", "EEMPTY", "EFIELDS", "EQNAME", "EFLAG", "ERNAME", "EPOS", "EMAPQ", "ECIGAR", "ERNEXT", "EPNEXT", "ETLEN", "ESEQ", "ECIGLEN", "EQUAL", "ETAG",
                 "ETAGRANGE", "ETAGFLOAT", "ETAGHEX", "EHDSQ", "EHDDUP"):
        assert f"#define PALACE_SAM_{name} {getattr(sc, name)} " in text, name
