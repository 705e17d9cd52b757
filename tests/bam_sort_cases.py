"""The rules of `bamsort` restated in Python from their text -- the sort key, the interval and bin a .bai files a
record under, the header rewrite, the stable sort of a record stream -- and generators of records, for the tests of
palace_amd/csrc/bam_sort.hip, bam_index.hip and the executable.  Nothing here comes from the code under test.  Test infrastructure."""
import random
import struct

from tests.test_host_bam_spec import aux_B, aux_i, aux_Z, cigar_words, record

REF_OPS = (0, 2, 3, 7, 8)                     # M D N = X consume the reference


def fields(rec: bytes):
    """a record's bytes (block_size word first) -> dict of the fixed fields"""
    tid, pos, l_name, mapq, bin_, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHI", rec, 4)
    return dict(tid=tid, pos=pos, l_name=l_name, n_cig=n_cig, flag=flag, l_seq=l_seq, bin=bin_)


def key_ok(rec: bytes, n_ref: int) -> bool:
    f = fields(rec)
    return -1 <= f["tid"] < n_ref and f["pos"] >= -1


def sort_key(rec: bytes, n_ref: int) -> int:
    f = fields(rec)
    t = n_ref if f["tid"] < 0 else f["tid"]
    return t << 33 | ((f["pos"] + 1) & 0xffffffff) << 1 | (f["flag"] >> 4 & 1)


def _aux_size(d, ty, v, end):
    ty = chr(ty)
    if ty in "AcC":
        return 1
    if ty in "sS":
        return 2
    if ty in "iIf":
        return 4
    if ty in "ZH":
        z = d.find(b"\0", v, end)
        return z - v + 1 if z >= 0 else 0
    if ty == "B":
        if end - v < 5:
            return 0
        es = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}.get(chr(d[v]), 0)
        return 5 + es * struct.unpack_from("<I", d, v + 1)[0] if es else 0
    return 0


def real_cigar(rec: bytes):
    """the op words of the CIGAR the record really has: its own, or the first CG:B,I tag's behind the <l_seq>S<ref>N placeholder"""
    f = fields(rec)
    at = 4 + 32 + f["l_name"]
    ops = list(struct.unpack_from(f"<{f['n_cig']}I", rec, at))
    if ops and f["tid"] >= 0 and f["pos"] >= 0 and ops[0] & 15 == 4 and ops[0] >> 4 == f["l_seq"]:
        x, end = at + 4 * f["n_cig"] + (f["l_seq"] + 1) // 2 + f["l_seq"], len(rec)
        while x + 3 <= end:
            v = x + 3
            sz = _aux_size(rec, rec[x + 2], v, end)
            if not sz or sz > end - v:
                break
            if rec[x:x + 2] == b"CG":
                if rec[x + 2] == ord("B") and rec[v] in b"Ii":
                    n = struct.unpack_from("<I", rec, v + 1)[0]
                    if f["n_cig"] <= n < (1 << 29):
                        ops = list(struct.unpack_from(f"<{n}I", rec, v + 5))
                break
            x = v + sz
    return ops


def span(rec: bytes):
    """[beg, end) a .bai files the record under"""
    f = fields(rec)
    n = 0 if f["flag"] & 4 else sum(w >> 4 for w in real_cigar(rec) if (w & 15) in REF_OPS)
    return f["pos"], f["pos"] + (n if n > 0 else 1)


def reg2bin(beg: int, end: int) -> int:
    """SAM specification 5.3"""
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


def indexable(rec: bytes) -> bool:
    b, e = span(rec)
    return b >= 0 and e <= 1 << 29


def sorted_records(recs, n_ref):
    """stable by the key (Python's sort is stable)"""
    return sorted(recs, key=lambda r: sort_key(r, n_ref))


def rewrite_text(text: str) -> str:
    if text.startswith("@HD\t"):
        eol = text.find("\n")
        line, rest = (text, "") if eol < 0 else (text[:eol], text[eol:])
        f = line.split("\t")
        for k in range(1, len(f)):
            if f[k].startswith("SO:"):
                f[k] = "SO:coordinate"
                break
        else:
            f.append("SO:coordinate")
        return "\t".join(f) + rest
    return "@HD\tVN:1.6\tSO:coordinate\n" + text


def split_records(stream: bytes, first: int):
    out, p = [], first
    while p < len(stream):
        n = 4 + struct.unpack_from("<I", stream, p)[0]
        out.append(stream[p:p + n])
        p += n
    assert p == len(stream)
    return out


def cg_record(name, flag, tid, pos, ops_text):
    """a record whose real CIGAR sits in the CG tag behind the placeholder"""
    ops = cigar_words(ops_text)
    l_seq = sum(w >> 4 for w in ops if (w & 15) in (0, 1, 4, 7, 8))
    ref = sum(w >> 4 for w in ops if (w & 15) in REF_OPS)
    return record(name, flag, tid, pos, 30, [(l_seq << 4) | 4, (ref << 4) | 3], l_seq=l_seq, aux=aux_i("NM", 1) + aux_B("CG", "I", ops))


def random_records(rng: random.Random, n: int, targets, unplaced: float = 0.05):
    """n records over `targets` [(name, length)]: forward and reverse, clips, deletions, long N spans, placed-unmapped mates, records
    without a CIGAR, CG placeholders, and records without a contig; every interval fits its target"""
    out = []
    for k in range(n):
        name = f"r{k}"
        if rng.random() < unplaced:
            out.append(record(name, 4 | (16 if rng.random() < 0.3 else 0), -1, -1, 0, "", l_seq=rng.randrange(0, 40)))
            continue
        tid = rng.randrange(len(targets))
        tlen = targets[tid][1]
        shape = rng.random()
        rev = 16 if rng.random() < 0.5 else 0
        if shape < 0.08:                                                    # a placed-unmapped mate: flag 0x4 with the mate's coordinates
            out.append(record(name, 4 | 1 | 8 * 0 | rev, tid, rng.randrange(tlen), 0, "", l_seq=rng.randrange(1, 60), mtid=tid, mpos=5))
            continue
        if shape < 0.12 and tlen > 120000:
            m = rng.randrange(10, 60)
            cig, ref = f"{m}M100000N{m}M", 2 * m + 100000
        elif shape < 0.16:
            cig, ref = f"{rng.randrange(1, 30)}S{rng.randrange(1, 30)}I", 0  # only S / I: no reference bases
        elif shape < 0.20:
            cig, ref = "", 0
        else:
            a, d, b = rng.randrange(1, 80), rng.randrange(0, 5), rng.randrange(1, 80)
            cig = f"{rng.randrange(1, 20)}S{a}M" + (f"{d}D" if d else "") + f"{b}M"
            ref = a + d + b
        pos = rng.randrange(0, max(1, tlen - max(ref, 1) + 1))
        if shape >= 0.96 and cig and ref:
            out.append(cg_record(name, rev, tid, pos, cig))
        else:
            out.append(record(name, rev, tid, pos, rng.randrange(61), cig, aux=aux_Z("XS", "x" * rng.randrange(0, 30)) if rng.random() < 0.5 else b""))
    return out
