"""The rules of `samview` restated in Python: one SAM line -> the bytes of its BAM record, DROPPED, or a PALACE_SAM_E*
code; the header; hand cases; and a seeded generator of valid and of damaged lines.  Nothing here comes from the device or from
csrc/sam_line.hpp: the tests compare them with this."""
import re
import struct

import numpy as np

DROPPED = "dropped"
(EAT, EEMPTY, EFIELDS, EQNAME, EFLAG, ERNAME, EPOS, EMAPQ, ECIGAR, ERNEXT, EPNEXT, ETLEN, ESEQ, ECIGLEN, EQUAL, ETAG, ETAGRANGE, ETAGFLOAT, ETAGHEX,
 EHDSQ, EHDDUP) = range(1, 22)
LINE_CODES = set(range(EAT, ETAGHEX + 1))
OPS = b"MIDNSHP=X"
NIBBLES = b"=ACMGRSVTWYHKDBN"
UDEC = re.compile(rb"[0-9]+\Z")
SDEC = re.compile(rb"-?[0-9]+\Z")
CIGAR = re.compile(rb"([0-9]+[MIDNSHP=X])+\Z")
B_RANGE = {b"c": (-128, 127), b"C": (0, 255), b"s": (-32768, 32767), b"S": (0, 65535), b"i": (-2**31, 2**31 - 1), b"I": (0, 2**32 - 1)}
B_FMT = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I"}


def reg2bin(beg, end):
    """SAM specification 5.3"""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def udec(f, hi):
    return int(f) if UDEC.match(f) and int(f) <= hi else None


def encode_tag(f):
    """-> bytes or a code"""
    if len(f) < 5 or f[2:3] != b":" or f[4:5] != b":" or not re.match(rb"[A-Za-z][A-Za-z0-9]\Z", f[:2]):
        return ETAG
    ty, v = f[3:4], f[5:]
    if ty == b"A":
        return f[:2] + b"A" + v if len(v) == 1 and 33 <= v[0] <= 126 else ETAG
    if ty == b"i":
        if not SDEC.match(v):
            return ETAG
        x = int(v)
        if not -2**31 <= x <= 2**32 - 1:
            return ETAGRANGE
        if x < 0:
            t = "b" if x >= -128 else "h" if x >= -32768 else "i"
        else:
            t = "B" if x <= 255 else "H" if x <= 65535 else "I"
        return f[:2] + {"b": b"c", "h": b"s", "i": b"i", "B": b"C", "H": b"S", "I": b"I"}[t] + struct.pack("<" + t, x)
    if ty == b"Z":
        return f[:2] + b"Z" + v + b"\0"
    if ty == b"H":
        return f[:2] + b"H" + v + b"\0" if len(v) % 2 == 0 and re.match(rb"[0-9A-Fa-f]*\Z", v) else ETAGHEX
    if ty == b"B":
        sub = v[:1]
        if sub == b"f":
            return ETAGFLOAT
        if sub not in B_RANGE:
            return ETAG
        vals, rest = [], v[1:]
        if rest:
            if rest[:1] != b",":
                return ETAG
            for item in rest[1:].split(b","):
                if not SDEC.match(item):
                    return ETAG
                if not B_RANGE[sub][0] <= int(item) <= B_RANGE[sub][1]:
                    return ETAGRANGE
                vals.append(int(item))
        return f[:2] + b"B" + sub + struct.pack("<i", len(vals)) + b"".join(struct.pack("<" + B_FMT[sub], x) for x in vals)
    if ty == b"f":
        return ETAGFLOAT
    return ETAG


def encode(line, targets, mask=0):
    """One alignment line (bytes, no LF); targets = the header's names (bytes) in order -> the record's bytes (block_size word
    included), DROPPED, or the first error's code in the order of the checks."""
    f = line.split(b"\t")
    if len(f) < 11:
        return EFIELDS
    tid_of = {n: k for k, n in enumerate(targets)}
    qname, flag_t, rname, pos_t, mapq_t, cigar, rnext, pnext_t, tlen_t, seq, qual = f[:11]
    codes = []
    if not (1 <= len(qname) <= 254 and all(33 <= c <= 126 for c in qname)):
        codes.append(EQNAME)
    flag = udec(flag_t, 65535)
    if flag is None:
        codes.append(EFLAG)
    tid = -1 if rname == b"*" else tid_of.get(rname)
    if tid is None:
        codes.append(ERNAME)
    pos1 = udec(pos_t, 2**31 - 1)
    if pos1 is None:
        codes.append(EPOS)
    mapq = udec(mapq_t, 255)
    if mapq is None:
        codes.append(EMAPQ)
    ops = []
    if cigar != b"*":
        if not CIGAR.match(cigar):
            codes.append(ECIGAR)
        else:
            ops = [(int(n), OPS.index(o)) for n, o in re.findall(rb"([0-9]+)([MIDNSHP=X])", cigar)]
            if len(ops) > 65535 or any(n >= 2**28 for n, _ in ops):
                codes.append(ECIGAR)
    mtid = -1 if rnext == b"*" else -2 if rnext == b"=" else tid_of.get(rnext)
    if mtid is None:
        codes.append(ERNEXT)
    pnext1 = udec(pnext_t, 2**31 - 1)
    if pnext1 is None:
        codes.append(EPNEXT)
    tlen = int(tlen_t) if SDEC.match(tlen_t) and -2**31 <= int(tlen_t) <= 2**31 - 1 else None
    if tlen is None:
        codes.append(ETLEN)
    if seq == b"":
        codes.append(ESEQ)
    l_seq = 0 if seq == b"*" else len(seq)
    if ops and seq != b"*" and sum(n for n, o in ops if o in (0, 1, 4, 7, 8)) != l_seq and ECIGAR not in codes:
        codes.append(ECIGLEN)
    if qual != b"*" and (qual == b"" or len(qual) != l_seq or not all(33 <= c <= 126 for c in qual)):
        codes.append(EQUAL)
    aux = b""
    for tag in f[11:]:
        t = encode_tag(tag)
        if isinstance(t, int):
            codes.append(t)
            break
        aux += t
    if codes:
        return codes[0]
    if flag & mask:
        return DROPPED
    pos = pos1 - 1
    if tid >= 0 and pos1 == 0:
        tid = -1                                     # "mapped query cannot have zero coordinate; treated as unmapped"
    if not ops:
        flag |= 4                                    # "mapped query must have a CIGAR; treated as unmapped"
    if mtid == -2:
        mtid = tid
    rlen = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    span = 1 if flag & 4 or rlen == 0 else rlen
    bin_ = 4680 if pos < 0 else reg2bin(pos, pos + span) & 0xffff
    packed = bytearray((l_seq + 1) // 2)
    for j, c in enumerate(seq if seq != b"*" else b""):
        k = NIBBLES.find(bytes([c]).upper())
        packed[j >> 1] |= (15 if k < 0 else k) << (0 if j & 1 else 4)
    q = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    body = struct.pack("<iiBBHHHIiii", tid, pos, len(qname) + 1, mapq, bin_, len(ops), flag, l_seq, mtid, pnext1 - 1, tlen)
    body += qname + b"\0" + b"".join(struct.pack("<I", n << 4 | o) for n, o in ops) + bytes(packed) + q + aux
    return struct.pack("<I", len(body)) + body


def split_lines(text):
    """the lines of a text: cut at LF, a last line without LF is a line"""
    lines = text.split(b"\n")
    return lines[:-1] if text.endswith(b"\n") or text == b"" else lines


def header_of(text):
    """-> (header text, header lines, [(name, length)]) or (code, line number)"""
    lines = split_lines(text)
    n_head, targets, seen = 0, [], set()
    for ln in lines:
        if not ln.startswith(b"@"):
            break
        n_head += 1
        f = ln.split(b"\t")
        if f[0] != b"@SQ":
            continue
        sn = next((x[3:] for x in f[1:] if x.startswith(b"SN:")), None)
        ln_t = next((x[3:] for x in f[1:] if x.startswith(b"LN:")), None)
        if not sn or ln_t is None or not UDEC.match(ln_t) or not 1 <= int(ln_t) <= 2**31 - 1:
            return EHDSQ, n_head
        if sn in seen:
            return EHDDUP, n_head
        seen.add(sn)
        targets.append((sn, int(ln_t)))
    head = b"".join(l + b"\n" for l in lines[:n_head])
    if n_head == len(lines) and n_head and not text.endswith(b"\n"):
        head = head[:-1]
    return head, n_head, targets


def bam_header(text):
    """the BAM header samview writes for `text` (SAM specification 4.2)"""
    head, _, targets = header_of(text)
    raw = b"BAM\1" + struct.pack("<i", len(head)) + head + struct.pack("<i", len(targets))
    for n, l in targets:
        raw += struct.pack("<i", len(n) + 1) + n + b"\0" + struct.pack("<i", l)
    return raw


def lines_verdict(text):
    """-> (header lines, alignment lines, first faulty line number or 0, its code or 0): the faults palace_sam_lines reports"""
    lines = split_lines(text)
    n_head = next((k for k, l in enumerate(lines) if not l.startswith(b"@")), len(lines))
    for k, l in enumerate(lines):
        if l == b"":
            return n_head, len(lines) - n_head, k + 1, EEMPTY
        if l.startswith(b"@") and k > n_head:
            return n_head, len(lines) - n_head, k + 1, EAT
    return n_head, len(lines) - n_head, 0, 0


def text_verdict(text, mask=0):
    """the whole text -> (records of the kept lines, sizes per alignment line (0: dropped), first faulty (line number, code) or None)"""
    n_head, _, line, code = lines_verdict(text)
    head = header_of(text)
    targets = [n for n, _ in head[2]]
    first = (line, code) if code else None
    recs, sizes = [], []
    for k, l in enumerate(split_lines(text)[n_head:]):
        if l == b"" or l.startswith(b"@"):
            sizes.append(0)
            continue
        r = encode(l, targets, mask)
        if isinstance(r, int):
            if first is None or n_head + k + 1 < first[0]:
                first = (n_head + k + 1, r)
            sizes.append(0)
        elif r is DROPPED:
            sizes.append(0)
        else:
            recs.append(r)
            sizes.append(len(r))
    return recs, sizes, first


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
TARGETS = [(b"ref", 45), (b"EDGE_2_length_900_cov_7.25", 900), (b"chr|odd:name", 2**31 - 1)]
HEADER = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % t for t in TARGETS) + b"@PG\tID:bwa\tPN:bwa\n"
NAMES = [n for n, _ in TARGETS]

# the reads of the SAM specification's section 1.1 example
SPEC_READS = [
    b"r001\t99\tref\t7\t30\t8M2I4M1D3M\t=\t37\t39\tTTAGATAAAGGATACTG\t*",
    b"r002\t0\tref\t9\t30\t3S6M1P1I4M\t*\t0\t0\tAAAAGATAAGGATA\t*",
    b"r003\t0\tref\t9\t30\t5S6M\t*\t0\t0\tGCCTAAGCTAA\t*\tSA:Z:ref,29,-,6H5M,17,0;",
    b"r004\t0\tref\t16\t30\t6M14N5M\t*\t0\t0\tATAGCTTCAGC\t*",
    b"r003\t2064\tref\t29\t17\t6H5M\t*\t0\t0\tTAGGC\t*\tSA:Z:ref,9,+,5S6M,30,1;",
    b"r001\t147\tref\t37\t30\t9M\t=\t7\t-39\tCAGCGGCAT\t*\tNM:i:1",
]
HAND_VALID = SPEC_READS + [
    b"pair/1\t73\tref\t12\t60\t5M\t=\t12\t0\tACGTN\tIIII#\tNM:i:0\tAS:i:-5\tXS:i:300\tMD:Z:5",
    b"pair/2\t133\tref\t12\t0\t*\t=\t12\t0\tacgtn\t!!~~5",                 # an unmapped mate that carries RNAME / POS
    b"zero\t0\tref\t0\t0\t4M\tEDGE_2_length_900_cov_7.25\t5\t-2147483648\tACGT\t*",      # an RNAME with POS 0
    b"nocig\t0\tchr|odd:name\t2147483647\t255\t*\t*\t0\t2147483647\t*\t*",
    b"tags\t4\t*\t0\t0\t*\t*\t0\t0\tRYKMSWBDHVN=.x\t*\tXA:A:!\tXH:H:\tXh:H:1aF0\tXZ:Z:\tZc:B:c\tZC:B:C,0,255\tZs:B:s,-32768,32767\tZS:B:S,65535\t"
    b"Zi:B:i,-2147483648,2147483647\tZI:B:I,4294967295\tXi:i:-0\tX0:i:007",
    b"allops\t16\tref\t3\t1\t1M1I1D1N1S1H1P1=1X\t*\t0\t0\tACGTA\tIIIII\tcr:Z:a b\r",
    b"odd\t0\tEDGE_2_length_900_cov_7.25\t16384\t7\t3M\t=\t1\t-16383\tTGA\tABC",
]
HAND_ERRORS = [
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA", EFIELDS), (b"\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EQNAME), (b"a b\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EQNAME),
    (b"a\t65536\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EFLAG), (b"a\t0x10\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EFLAG), (b"a\t-0\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EFLAG),
    (b"a\t\tref\t1\t0\t1M\t*\t0\t0\tA\t*", EFLAG), (b"a\t0\tnone\t1\t0\t1M\t*\t0\t0\tA\t*", ERNAME), (b"a\t0\t\t1\t0\t1M\t*\t0\t0\tA\t*", ERNAME),
    (b"a\t0\t=\t1\t0\t1M\t*\t0\t0\tA\t*", ERNAME), (b"a\t0\tref\t+1\t0\t1M\t*\t0\t0\tA\t*", EPOS), (b"a\t0\tref\t1\t256\t1M\t*\t0\t0\tA\t*", EMAPQ),
    (b"a\t0\tref\t1\t0\tM\t*\t0\t0\tA\t*", ECIGAR), (b"a\t0\tref\t1\t0\t1\t*\t0\t0\tA\t*", ECIGAR), (b"a\t0\tref\t1\t0\t1M1\t*\t0\t0\tA\t*", ECIGAR),
    (b"a\t0\tref\t1\t0\t1m\t*\t0\t0\tA\t*", ECIGAR), (b"a\t0\tref\t1\t0\t\t*\t0\t0\tA\t*", ECIGAR), (b"a\t0\tref\t1\t0\t268435456M\t*\t0\t0\t*\t*", ECIGAR),
    (b"a\t0\tref\t1\t0\t1M\tnone\t0\t0\tA\t*", ERNEXT), (b"a\t0\tref\t1\t0\t1M\t*\t-1\t0\tA\t*", EPNEXT), (b"a\t0\tref\t1\t0\t1M\t*\t0\t2147483648\tA\t*", ETLEN),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t--1\tA\t*", ETLEN), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\t\t*", ESEQ), (b"a\t0\tref\t1\t0\t2M\t*\t0\t0\tA\t*", ECIGLEN),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\tII", EQUAL), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t ", EQUAL), (b"a\t0\tref\t1\t0\t*\t*\t0\t0\t*\tI", EQUAL),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t", EQUAL), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\t", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tN:i:1", ETAG),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\t1M:i:1", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tNM:i:", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tNM:i:+1", ETAG),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tNM:I:1", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tXA:A:ab", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tXA:A:", ETAG),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:c,", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:c1", ETAG),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:C,-1", ETAGRANGE), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:c,128,x", ETAGRANGE),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:c,1,x,128", ETAG), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tXF:f:1.5", ETAGFLOAT),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tZB:B:f,1.5", ETAGFLOAT), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tXH:H:abc", ETAGHEX),
    (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tXH:H:0g", ETAGHEX), (b"a\t0\tref\t1\t0\t1M\t*\t0\t0\tA\t*\tNM:i:1\tXF:f:1\tXH:H:a", ETAGFLOAT),
    # several faults: the first in the order of the checks
    (b"a\t0\tnone\t1\t0\t1\tnone\t0\t0\tA\tII\tXF:f:1", ERNAME), (b"a\t0\tref\t1\t0\t1\tnone\t0\t0\tA\tII", ECIGAR), (b"a\t0\tref\t1\t0\t2M\t*\t0\t0\tA\tII", ECIGLEN),
]
INT_BORDERS = [(-2147483649, ETAGRANGE), (-2147483648, b"i"), (-32769, b"i"), (-32768, b"s"), (-129, b"s"), (-128, b"c"), (-1, b"c"), (0, b"C"), (255, b"C"),
               (256, b"S"), (65535, b"S"), (65536, b"I"), (4294967295, b"I"), (4294967296, ETAGRANGE)]


def random_name(rng, n):
    return bytes(rng.integers(33, 127, size=n).astype(np.uint8)).replace(b"@", b"a")


def valid_line(rng, seq_len=None):
    """a valid line with every tag type among its tags now and then, '*' wherever it may stand, all nine ops"""
    l_seq = int(rng.integers(1, 140)) if seq_len is None else seq_len
    star_seq = seq_len is None and rng.random() < 0.1
    if star_seq:
        l_seq = 0
    cigar = b"*"
    if rng.random() < 0.85:
        if star_seq:
            cigar = b"".join(b"%d%c" % (int(rng.integers(0, 300)), OPS[int(rng.integers(0, 9))]) for _ in range(int(rng.integers(1, 6))))
        else:                                                                # query ops that sum to l_seq, the others in between
            cuts = sorted(set(int(x) for x in rng.integers(0, l_seq + 1, size=int(rng.integers(0, 5)))) | {0, l_seq})
            parts = []
            for a, b in zip(cuts, cuts[1:]):
                parts.append(b"%d%c" % (b - a, b"MIS=X"[int(rng.integers(0, 5))]))
                if rng.random() < 0.5:
                    parts.append(b"%d%c" % (int(rng.integers(0, 2000)), b"DNHP"[int(rng.integers(0, 4))]))
            cigar = b"".join(parts) if parts else b"0M"
            if l_seq == 0:
                cigar = b"3D"
    seq = b"*" if star_seq or (l_seq == 0) else bytes(rng.choice(np.frombuffer(b"ACGTNacgtn=RYKMSWBDHV.x", np.uint8), size=l_seq))
    if seq == b"*":
        l_seq = 0
    if cigar != b"*" and seq == b"*" and rng.random() < 0.5:
        cigar = b"*"
    qual = b"*" if rng.random() < 0.3 or l_seq == 0 else bytes(rng.integers(33, 127, size=l_seq).astype(np.uint8))
    rname = NAMES[int(rng.integers(0, 3))] if rng.random() < 0.85 else b"*"
    rnext = [b"*", b"=", NAMES[int(rng.integers(0, 3))]][int(rng.integers(0, 3))]
    tags = []
    for _ in range(int(rng.integers(0, 7))):
        name = bytes([rng.choice(np.frombuffer(b"XYZNMAS", np.uint8)), rng.choice(np.frombuffer(b"AMSZ019az", np.uint8))])
        k = int(rng.integers(0, 6))
        if k == 0:
            tags.append(name + b":A:" + bytes([int(rng.integers(33, 127))]))
        elif k == 1:
            span = [200, 40000, 2**31, 2**32][int(rng.integers(0, 4))]
            tags.append(name + b":i:%d" % int(rng.integers(-min(span, 2**31), span)))
        elif k == 2:
            tags.append(name + b":Z:" + bytes(rng.integers(32, 127, size=int(rng.integers(0, 90))).astype(np.uint8)))
        elif k == 3:
            tags.append(name + b":H:" + bytes(rng.choice(np.frombuffer(b"0123456789abcdefABCDEF", np.uint8), size=2 * int(rng.integers(0, 9)))))
        else:
            sub = b"cCsSiI"[int(rng.integers(0, 6)):][:1]
            lo, hi = B_RANGE[sub]
            tags.append(name + b":B:" + sub + b"".join(b",%d" % int(rng.integers(lo, hi + 1)) for _ in range(int(rng.integers(0, 6)))))
    flag = int(rng.integers(0, 65536)) if rng.random() < 0.5 else int(rng.choice([0, 16, 4, 99, 147, 2048, 2064, 256]))
    f = [random_name(rng, int(rng.integers(1, 40))), b"%d" % flag, rname, b"%d" % int(rng.integers(0, 900) if rng.random() < 0.9 else rng.integers(0, 2**31)),
         b"%d" % int(rng.integers(0, 256)), cigar, rnext, b"%d" % int(rng.integers(0, 2000)), b"%d" % int(rng.integers(-3000, 3000)), seq, qual] + tags
    return b"\t".join(f)


DAMAGE = [
    (lambda f, r: f[:int(r.integers(1, 11))], EFIELDS), (lambda f, r: [b"q\x7fname"] + f[1:], EQNAME), (lambda f, r: [b"n" * 255] + f[1:], EQNAME),
    (lambda f, r: f[:1] + [b"70000"] + f[2:], EFLAG), (lambda f, r: f[:2] + [b"nowhere"] + f[3:], ERNAME), (lambda f, r: f[:3] + [b"2147483648"] + f[4:], EPOS),
    (lambda f, r: f[:4] + [b"3.5"] + f[5:], EMAPQ), (lambda f, r: f[:5] + [b"5M3"] + f[6:], ECIGAR), (lambda f, r: f[:5] + [b"5Q"] + f[6:], ECIGAR),
    (lambda f, r: f[:6] + [b"ref2"] + f[7:], ERNEXT), (lambda f, r: f[:7] + [b""] + f[8:], EPNEXT), (lambda f, r: f[:8] + [b"1e3"] + f[9:], ETLEN),
    (lambda f, r: f[:9] + [b""] + f[10:], ESEQ), (lambda f, r: f[:5] + [b"%dM" % (len(f[9]) + 1), f[6], f[7], f[8], f[9] if f[9] != b"*" else b"A", b"*"] + f[11:], ECIGLEN),
    (lambda f, r: f[:10] + [f[10] + b"I" if f[10] != b"*" else b"II" + b"I" * len(f[9])] + f[11:], EQUAL), (lambda f, r: f[:11] + [b"X:Z:short"] + f[11:], ETAG),
    (lambda f, r: f[:11] + [b"XX:i:4294967296"] + f[11:], ETAGRANGE), (lambda f, r: f[:11] + [b"XS:B:s,32768"] + f[11:], ETAGRANGE),
    (lambda f, r: f[:11] + [b"XF:f:0.25"] + f[11:], ETAGFLOAT), (lambda f, r: f[:11] + [b"XH:H:abc"] + f[11:], ETAGHEX),
]


def generated(seed, n, damaged=0.35):
    """n lines: valid ones, and ones with one field broken each; besides them an empty line and an '@' line now and then"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        x = rng.random()
        if x < 0.01:
            out.append(b"")
        elif x < 0.02:
            out.append(b"@CO\tlate")
        elif x < damaged:
            fn, _ = DAMAGE[int(rng.integers(0, len(DAMAGE)))]
            out.append(b"\t".join(fn(valid_line(rng).split(b"\t"), rng)))
        else:
            out.append(valid_line(rng))
    return out
