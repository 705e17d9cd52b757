"""The grammar of a `samtools depth` line restated in Python, and the case table the depth-file tests share (the reference of
tests/test_host_depth_line.py, tests/test_gpu_depth_parse.py and tests/test_gpu_bamdepth_from_depth.py: never the code under test)."""
import numpy as np

VMAX = 2 ** 31 - 1


def parse_line(b: bytes):
    """(name, position, depth) of a line without its LF, or None when it is not `name<TAB>1-10 digits<TAB>1-10 digits`"""
    f = b.split(b"\t")
    if len(b) > 4095 or len(f) != 3 or not f[0] or b"\n" in b:
        return None
    for x in f[1:]:
        if not 1 <= len(x) <= 10 or any(c not in b"0123456789" for c in x) or int(x) > VMAX:
            return None
    return f[0], int(f[1]), int(f[2])


def lines_of(text: bytes):
    ls = text.split(b"\n")
    return ls[:-1] if ls[-1] == b"" else ls          # the empty text behind a final LF is not a line


def restate(text: bytes):
    """-> (first bad line number or 0, lines, depth sum, {name: [sum, lines]} in order of first appearance, maximal runs [name, sum, lines])"""
    per, runs, total = {}, [], 0
    ls = lines_of(text)
    for i, l in enumerate(ls, 1):
        p = parse_line(l)
        if p is None:
            return i, len(ls), None, None, None
        total += p[2]
        e = per.setdefault(p[0], [0, 0])
        e[0] += p[2]
        e[1] += 1
        if not runs or runs[-1][0] != p[0]:
            runs.append([p[0], 0, 0])
        runs[-1][1] += p[2]
        runs[-1][2] += 1
    return 0, len(ls), total, per, runs


def awk_number(total: int, n: int) -> bytes:
    v = total / n
    return b"%d" % int(v) if v == int(v) and abs(v) < 1e15 else b"%.6g" % v


GOOD = [b"a\t1\t1", b"n" * 4000 + b"\t5\t7", b"c\t10\t0", b"c\t11\t2147483647", b"c\t0000000012\t0000000003", b"c\t2147483647\t0000000000",
        b"a b #x \xc3\xa9\xff\t3\t4", b"#c\t1\t1"]
BAD = [b"", b"\t1\t1", b"abc", b"abc\t1", b"abc\t1\t2\t3", b"abc\t\t2", b"abc\t1\t", b"abc\t-1\t2", b"abc\t1\t+2", b"abc\t1\t2\r", b"abc\t1 \t2",
       b"abc\t1\t 2", b"abc\t00000000001\t2", b"abc\t1\t12345678901", b"abc\t2147483648\t1", b"abc\t1\t2147483648", b"x" * 4092 + b"\t1\t1",
       b"# a header line"]
assert all(parse_line(l) is not None for l in GOOD) and all(parse_line(l) is None for l in BAD) and len(BAD[-2]) == 4096


def random_lines(rng, n):
    out = []
    for _ in range(n):
        k = int(rng.integers(0, 10))
        if k < 5:
            name = bytes(rng.integers(33, 127, size=int(rng.integers(1, 30)), dtype=np.uint8).tolist())
            out.append(b"%s\t%d\t%d" % (name, int(rng.integers(0, VMAX + 1)), int(rng.integers(0, VMAX + 1))))
        elif k < 7:
            out.append(GOOD[int(rng.integers(0, len(GOOD)))])
        elif k < 9:
            out.append(BAD[int(rng.integers(0, len(BAD)))])
        else:                                       # printable noise with tabs and digits: mostly bad, sometimes not
            out.append(bytes(rng.choice(np.frombuffer(b"ab\t\t019 -", dtype=np.uint8), size=int(rng.integers(0, 12))).tolist()))
    return out
