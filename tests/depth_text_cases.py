"""The depth stage restated for the ABI tests of csrc/depth.hip and csrc/depth_text.hip: plain numpy and Python, nothing of the code
under test.  A case is contigs (lengths, names) and match segments (tid, pos, len: int32, possibly nonsense); `Reference` is what
the five entry points have to say about it.

The rule for one segment (all arithmetic in int64 / Python ints): dropped if tid < 0, tid >= n_targets, pos < 0, len <= 0 or
min(pos + len, tlen[tid]) <= pos; otherwise it covers [pos, min(pos + len, tlen[tid])) of its contig."""
from types import SimpleNamespace

import numpy as np

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
TILE = 1024                                  # positions per tile of depth_text.hip
EMIT_GRID = 4096                             # workgroups of one emit launch: more tiles than this between two covered ones -> its stride loop


def make_case(tlen, names, segs, **more):
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 3)
    assert segs.size == 0 or (segs.min() >= I32_MIN and segs.max() <= I32_MAX)
    assert len(tlen) == len(names)
    return SimpleNamespace(tlen=[int(x) for x in tlen], names=[bytes(x) for x in names], segs=np.ascontiguousarray(segs.astype(np.int32)), **more)


def kept_segments(tlen, segs):
    """-> (tid, first, end) int64 arrays of the segments that count, each cut at its contig's end"""
    s = np.asarray(segs).astype(np.int64).reshape(-1, 3)
    tl = np.asarray(tlen, dtype=np.int64)
    tid, pos, ln = s[:, 0], s[:, 1], s[:, 2]
    ok = (tid >= 0) & (tid < len(tl)) & (pos >= 0) & (ln > 0)
    tid, pos, ln = tid[ok], pos[ok], ln[ok]
    end = np.minimum(pos + ln, tl[tid]) if len(tid) else pos
    ok = end > pos
    return tid[ok], pos[ok], end[ok]


class Reference:
    def __init__(self, tlen, names, segs):
        tlen = [int(x) for x in tlen]
        self.n_targets, self.total_len = len(tlen), sum(tlen)
        self.tbase = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(tlen, dtype=np.int64))])
        tid, a, b = kept_segments(tlen, segs)
        order = np.argsort(tid, kind="stable")
        tid, a, b = tid[order], a[order], b[order]
        cut = np.searchsorted(tid, np.arange(self.n_targets + 1))
        self.contig_sum, self.contig_covered = np.zeros(self.n_targets, np.uint64), np.zeros(self.n_targets, np.uint64)
        parts, lens, gpos = [], [], []
        for t in range(self.n_targets):
            if cut[t] == cut[t + 1]:
                continue
            L = tlen[t]
            diff = (np.bincount(a[cut[t]:cut[t + 1]], minlength=L + 1) - np.bincount(b[cut[t]:cut[t + 1]], minlength=L + 1)).astype(np.int64)
            depth = np.cumsum(diff[:-1])
            assert diff.sum() == 0 and (depth >= 0).all()
            pos = np.flatnonzero(depth > 0)
            dep = depth[pos]
            self.contig_sum[t], self.contig_covered[t] = int(dep.sum()), len(pos)
            name = bytes(names[t])
            mine = [name + b"\t%d\t%d\n" % pd for pd in zip((pos + 1).tolist(), dep.tolist())]
            parts.append(b"".join(mine))
            lens.append(np.fromiter(map(len, mine), dtype=np.int64, count=len(mine)))
            gpos.append(pos + self.tbase[t])
        self.text = b"".join(parts)
        lens = np.concatenate(lens) if lens else np.zeros(0, np.int64)
        self.line_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)])           # lines + 1 entries: the last = len(text)
        self.line_g = np.concatenate(gpos) if gpos else np.zeros(0, np.int64)              # the global position of each line
        self.lines, self.sum = len(self.line_g), int(self.contig_sum.sum())
        assert self.sum == int((b - a).sum()) and self.line_off[-1] == len(self.text)

    def text_lines(self):
        return [self.text[a:b] for a, b in zip(self.line_off[:-1].tolist(), self.line_off[1:].tolist())]

    def windows_reference(self, beg, end):
        """-> (text_beg[], text_end[], lines[]) as uint64, for ranges of global positions of any kind"""
        g0 = np.maximum(0, np.asarray(beg, dtype=np.int64))
        g1 = np.maximum(g0, np.asarray(end, dtype=np.int64))
        i0, i1 = np.searchsorted(self.line_g, g0, side="left"), np.searchsorted(self.line_g, g1, side="left")
        return self.line_off[i0].astype(np.uint64), self.line_off[i1].astype(np.uint64), (i1 - i0).astype(np.uint64)


def reference(case) -> Reference:
    return Reference(case.tlen, case.names, case.segs)


def global_segments(tlen, g0, g1):
    """segments that cover the global positions [g0, g1), one per contig touched"""
    out, base = [], 0
    for t, L in enumerate(tlen):
        lo, hi = max(g0, base), min(g1, base + L)
        if hi > lo:
            out.append((t, lo - base, hi - lo))
        base += L
    return out


# ---- (a) tile geometry ------------------------------------------------------------------------------------------------------------------
GEOMETRY_TOTALS = [1, 1023, 1024, 1025, 2048, 256 * 1024, 256 * 1024 + 1, 257 * 1024 + 5]
GEOMETRY_PATTERNS = ["nothing", "first", "last", "borders", "one_segment", "segment_per_position"]


def geometry_case(total, pattern, split):
    """one contig of `total` positions, or the same positions as two contigs cut at 1024 (the second one empty up to there)"""
    tlen = [min(total, TILE), total - min(total, TILE)] if split else [total]
    names = [b"left", b"right_of_1024"] if split else [b"only"]
    if pattern == "nothing":
        spans = []
    elif pattern == "first":
        spans = [(0, 1)]
    elif pattern == "last":
        spans = [(total - 1, total)]
    elif pattern == "borders":                # the two positions on either side of every tile border
        spans = [(g, g + 1) for k in range(TILE, total + 1, TILE) for g in (k - 1, k) if g < total]
    elif pattern == "one_segment":
        spans = [(0, total)]
    else:
        spans = [(g, g + 1) for g in range(total)]
    if len(spans) > 64:                       # single positions: contig by contig without the walk of global_segments
        g = np.asarray([s[0] for s in spans], dtype=np.int64)
        right = g >= tlen[0]
        segs = np.stack([right.astype(np.int64), g - right * tlen[0], np.ones(len(g), np.int64)], axis=1)
    else:
        segs = [s for g0, g1 in spans for s in global_segments(tlen, g0, g1)]
    return make_case(tlen, names, segs)


# ---- (b) depth digit steps --------------------------------------------------------------------------------------------------------------
DEPTH_STEPS = [1, 9, 10, 99, 100, 999, 1000, 9_999, 10_000, 99_999, 100_000, 999_999, 1_000_000]


def depth_digits_case(staggered):
    """one contig of 64 positions per k of DEPTH_STEPS with k segments on it: all [5, 40), or segment i = [i mod 7, 40), so that
    the depths of positions 0..6 climb through the digit step inside one thread's four positions"""
    tlen, names, segs = [64] * len(DEPTH_STEPS), [b"k%d" % k for k in DEPTH_STEPS], []
    for t, k in enumerate(DEPTH_STEPS):
        first = np.arange(k, dtype=np.int64) % 7 if staggered else np.full(k, 5, np.int64)
        segs.append(np.stack([np.full(k, t, np.int64), first, 40 - first], axis=1))
    return make_case(tlen, names, np.concatenate(segs))


# ---- (c) position digit steps, far apart ------------------------------------------------------------------------------------------------
LONG_CONTIG = 10_000_001


def position_digits_case():
    """a short contig, then one of 10 000 001 positions with the 1-based positions (9, 10), (99, 100) ... (9 999 999, 10 000 000)
    and the last one covered: the covered tiles lie further apart than one emit launch has workgroups"""
    tlen, names = [7, LONG_CONTIG], [b"s", b"long_contig_with_a_name_of_forty_bytes__"]
    assert len(names[1]) == 40
    segs = [(0, 3, 1)] + [(1, 10 ** e - 2, 2) for e in range(1, 8)] + [(1, LONG_CONTIG - 1, 1)]
    return make_case(tlen, names, segs)


def covered_tiles(ref):
    return np.unique(ref.line_g // TILE)


# ---- (d), (e) contig geometry and segments that do not count ------------------------------------------------------------------------------
CONTIG_CYCLE = [0, 1, 2, 3, 5, 63, 64, 65, 127, 1024]


def ignored_segments(tlen, t):
    """the segments of (e) around contig t (tlen[t] > 0): all dropped but the one from the last base with len = INT32_MAX, which is
    cut to that base"""
    L, n = tlen[t], len(tlen)
    return [(-1, 0, 5), (n, 0, 5), (I32_MIN, 0, 5), (t, -1, 5), (t, 0, 0), (t, 1, -5), (t, L, 3), (t, L - 1, I32_MAX), (t, I32_MAX - 1, I32_MAX)]


def contig_case(with_long=False, with_ignored=False, shuffle_seed=None):
    """300 contigs of the lengths of CONTIG_CYCLE (several inside one thread's four positions), an empty contig first, last and on a
    tile border, names of 1, 40 and 255 bytes (bytes >= 0x80 and a space among them, one name twice), short segments at every contig's
    ends, and for the bitmap of depth.hip a segment that fills an aligned 64-bit word and single positions at bits 63 and 0"""
    tlen = [CONTIG_CYCLE[i % len(CONTIG_CYCLE)] for i in range(300)]
    pad = -sum(tlen) % TILE
    tlen += [pad, 0, 200]                                                  # the empty contig 301 starts (and ends) on a tile border
    assert pad > 0 and sum(tlen[:301]) % TILE == 0 and tlen[0] == 0
    if with_long:
        tlen.append(1_000_000)
    tlen.append(0)
    n = len(tlen)
    names = []
    for t in range(n):
        if t % 50 == 7:
            names.append(bytes([0x80 + (t + j) % 0x20 for j in range(254)]) + b" ")             # 255 bytes, 0x80..0x9f and a space
        elif t % 10 == 3:
            names.append(b"ctg %03d \xc3\xa9\xff" % t + b"x" * 29)                               # 40 bytes
        else:
            names.append(bytes([33 + t % 90]))                                                    # 1 byte: names repeat
    if with_long:
        names[n - 2] = b"L"                                                                        # (a million lines of it)
    names[20] = names[13]                                                                          # a 40-byte name twice
    assert {len(x) for x in names} == {1, 40, 255} and all(b"\t" not in x and b"\n" not in x and 0xA5 not in x for x in names)
    base = np.concatenate([[0], np.cumsum(tlen)]).tolist()
    segs = []
    for t in range(n):
        L = tlen[t]
        if L == 0:
            continue
        segs.append((t, max(0, L - 2), 2 if L > 1 else 1))                 # ends on the last base
        if t % 3 == 0:
            segs.append((t, 0, 1))                                         # starts at 0 behind the contig before
        if t % 4 == 1:
            segs.append((t, L - 1, 7))                                     # runs past the end: cut
        if L == 1024 and t % 100 == 9:
            g = -(-(base[t] + 100) // 64) * 64                             # an aligned 64-bit word of the bitmap, filled exactly
            segs.append((t, g - base[t], 64))
            segs.append((t, g + 127 - base[t], 1))                         # bit 63 of a word, alone
            segs.append((t, g + 256 - base[t], 1))                         # bit 0 of a word, alone
    last = max(t for t in range(n) if tlen[t] > 0)
    segs.append((last, tlen[last] - 3, 3))                                 # ends exactly at total_len
    if with_long:
        segs.append((n - 2, 0, 1_000_000))
    if with_ignored:
        for t in (1, 9, 299, last):
            segs += ignored_segments(tlen, t)
    segs = np.asarray(segs, dtype=np.int64)
    if shuffle_seed is not None:
        segs = segs[np.random.default_rng(shuffle_seed).permutation(len(segs))]
    return make_case(tlen, names, segs)


def ignored_alone_case(with_cut):
    """the segments of (e) on their own: without the one that is cut to its contig's last base, nothing at all is covered"""
    tlen, names = [0, 5, 1024, 0, 70], [b"e0", b"five", b"tile", b"e3", b"seventy"]
    segs = [s for t in (1, 2, 4) for s in ignored_segments(tlen, t) if with_cut or s[2] != I32_MAX or s[1] != tlen[t] - 1]
    return make_case(tlen, names, segs)


# ---- (g) a text whose covered tiles have empty tiles between them -------------------------------------------------------------------------
def sparse_tiles_case():
    tlen, names = [3 * TILE + 10, 0, 17 * TILE], [b"front", b"none", b"tail contig"]
    spans = [(1000, 1030), (5 * TILE - 2, 5 * TILE + 3), (6 * TILE, 6 * TILE + 4), (11 * TILE + 500, 11 * TILE + 520), (19 * TILE - 1, 19 * TILE + 1),
             (sum(tlen) - 2, sum(tlen))]
    segs = [s for g0, g1 in spans for s in global_segments(tlen, g0, g1)] + [(2, 5 * TILE - 3 * TILE - 10, 2)]
    return make_case(tlen, names, segs)


def emit_ranges(ref, n_lines=40, n_single=600, n_random=300, seed=11):
    """the ranges of (g): all [s, e) with s <= e among {line start, line start - 1, line start + 1, first digit of the position, the
    LF} of n_lines lines -- the first and last line of every covered tile first, the rest spread evenly --, single bytes, random
    ranges, the whole text and a range inside one line's name"""
    n, size = ref.lines, len(ref.text)
    tile = ref.line_g // TILE
    edge = np.flatnonzero(np.concatenate([[True], tile[1:] != tile[:-1]]) | np.concatenate([tile[1:] != tile[:-1], [True]]))
    starts = ref.line_off[:-1].tolist()
    longest = max(range(n), key=lambda i: ref.text.index(b"\t", starts[i]) - starts[i])          # a line with the longest name
    chosen = list(dict.fromkeys([longest] + edge.tolist()[:n_lines // 2] + [0, n - 1] + np.linspace(0, n - 1, n_lines).astype(int).tolist()))[:n_lines]
    names_end = {}
    points = set()
    for i in chosen:
        s, e = int(ref.line_off[i]), int(ref.line_off[i + 1])
        tab = ref.text.index(b"\t", s, e)
        names_end[i] = tab
        points |= {s, max(s - 1, 0), s + 1, tab + 1, e - 1}
    points = sorted(points)
    ranges = [(a, b) for k, a in enumerate(points) for b in points[k:]]
    ranges += [(a, a + 1) for a in range(min(n_single, size))]
    rng = np.random.default_rng(seed)
    ab = np.sort(rng.integers(0, size + 1, size=(n_random, 2)), axis=1)
    ranges += [(int(a), int(b)) for a, b in ab] + [(0, size)]
    s, e = starts[longest], names_end[longest]                             # inside one line's name
    ranges.append((s + 1, e - 1) if e - s > 2 else (s, e))
    return ranges


# ---- (h) ranges of positions for `windows` ------------------------------------------------------------------------------------------------
def window_ranges(ref, n_random, seed=5):
    """-> (special ranges, random ranges) as int64 (n, 2) arrays"""
    T = ref.total_len
    first, last = (int(ref.line_g[0]), int(ref.line_g[-1])) if ref.lines else (0, 0)
    sp = [(5, 5), (T // 2, T // 2), (40, 10), (T, 0), (-7, 30), (-(1 << 40), T), (I32_MIN, -1), (0, T + 1), (T - 10, T + (1 << 40)), (0, 1 << 62),
          (T, T + 5), (T + 1, T + 2), (1 << 50, 1 << 51), (0, T), (0, 0), (T - 1, T), (first, first + 1), (first, last + 1), (last + 1, T),
          (last + 1, last + 1), (last, last + 1), (first + 1, last)]
    for k in list(range(TILE, min(T, 6 * TILE) + 1, TILE)) + [k for k in (100 * TILE, 255 * TILE, 256 * TILE, 257 * TILE) if 6 * TILE < k <= T]:
        sp += [(k, k + 3), (k - 1, k + 1), (k + 1, k + TILE), (k - TILE, k), (k, k + 3 * TILE)]
    sp += [(T // TILE * TILE, T), (T // TILE * TILE - 1, T), (T // TILE * TILE + 1, T)]
    for t in range(0, ref.n_targets - 12, max(1, ref.n_targets // 7)):     # several contigs, the empty ones and empty tiles among them
        sp.append((int(ref.tbase[t]), int(ref.tbase[t + 12])))
        sp.append((int(ref.tbase[t]) + 1, int(ref.tbase[t + 11]) - 1))
    rng = np.random.default_rng(seed)
    rnd = np.sort(rng.integers(0, T + 1, size=(n_random, 2)), axis=1)
    near = rng.integers(0, max(ref.lines, 1), size=n_random // 2)          # half of them begin at or next to a covered position
    if ref.lines:
        rnd[:len(near), 0] = ref.line_g[near] + rng.integers(-1, 2, size=len(near))
        rnd[:len(near), 1] = rnd[:len(near), 0] + rng.integers(0, 3000, size=len(near))
    return np.asarray(sp, dtype=np.int64), rnd.astype(np.int64)
