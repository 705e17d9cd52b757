"""The arithmetic of a .bai restated in Python from the comment blocks of include/palace_hip.h (palace_bai_records, palace_bai_chunks,
palace_bai_linear, palace_bgzf_voffsets) and DESIGN.md section 8, on top of the record rules of tests/bam_sort_cases.py: the reference
that judges palace_amd/csrc/bam_index.hip at the ABI (tests/test_gpu_bai_abi.py), itself pinned to the reader's side of the format by
tests/test_host_bai_reference.py.  Integers only.  Nothing here comes from the code under test.  Test infrastructure."""
import struct
from bisect import bisect_right
from collections import namedtuple

import numpy as np

from tests import bam_sort_cases as bc

PSEUDO_BIN = 37450
NONE = 2 ** 64 - 1                             # the virtual offset of a stream offset outside the member table

Columns = namedtuple("Columns", "ref bin win_beg win_end unmapped bad status")
Linear = namedtuple("Linear", "n_intv n_mapped n_unmapped first last used lin_off lin")


def starts_and_sizes(recs, first):
    """record starts as palace_bam_walk leaves them (behind the block_size word) and the block_size words, for records laid out one
    behind the other from stream offset `first`"""
    sizes = np.array([len(r) - 4 for r in recs], dtype=np.int64)
    starts = first + 4 + np.concatenate(([0], np.cumsum(sizes + 4)[:-1])).astype(np.int64) if len(recs) else np.zeros(0, np.int64)
    return starts, sizes


FORCED_REFS = (0, 1, 255, 256, 257, 65535, 65536, 65537, 69999)              # around the per-reference kernels' workgroup of 256 and bit 16 of the run key
EMPTY_STRETCHES = ((2000, 3000), (66000, 67000))                            # references that stay without records


def many_reference_records(rng, n_ref, n_others, tlen, n_unplaced):
    """records (unsorted) on FORCED_REFS and on n_others random references outside EMPTY_STRETCHES, 1 to 40 per reference and mostly
    few, every reference `tlen` long: plain matches, spliced ones over several 16 kb windows, placed-unmapped mates; n_unplaced
    records without a contig -> (records, the used references sorted)"""
    assert n_ref > max(FORCED_REFS) and tlen > 50000
    free = [t for t in range(n_ref) if t not in FORCED_REFS and not any(a <= t < b for a, b in EMPTY_STRETCHES)]
    used = sorted(set(FORCED_REFS) | set(rng.sample(free, n_others)))
    recs = []
    for t in used:
        for k in range(40 if t in (0, 65536) else 1 + int(39 * rng.random() ** 10)):
            name, rev, shape = f"t{t}_{k}", 16 * rng.randrange(2), rng.random()
            if shape < 0.1:
                recs.append(bc.record(name, 4 | 1 | rev, t, rng.randrange(tlen), 0, "", l_seq=rng.randrange(1, 40), mtid=t, mpos=7))
            elif shape < 0.2:
                recs.append(bc.record(name, rev, t, rng.randrange(tlen - 40040), 60, "20M40000N20M"))
            else:
                m = rng.randrange(1, 120)
                recs.append(bc.record(name, rev, t, rng.randrange(tlen - m + 1), rng.randrange(61), f"{rng.randrange(1, 9)}S{m}M"))
    recs += [bc.record(f"u{k}", 4, -1, -1, 0, "", l_seq=rng.randrange(0, 30)) for k in range(n_unplaced)]
    rng.shuffle(recs)
    return recs, used


def columns(recs, n_ref):
    """what each record is filed under, and the four status numbers (n_bad, first_bad, first_unsorted, n_no_coor).  `bad` marks the
    records a .bai cannot hold: their columns other than `unmapped` are unspecified (zeros here, not to be compared).  A record
    without a contig has ref = -1 and bin = win_beg = win_end = 0."""
    n = len(recs)
    ref, bin_, wb, we = (np.zeros(n, np.int32) for _ in range(4))
    unm, bad = np.zeros(n, np.uint8), np.zeros(n, bool)
    n_no_coor, first_unsorted, prev_key = 0, -1, None
    for i, r in enumerate(recs):
        f = bc.fields(r)
        unm[i] = 1 if f["flag"] & 4 else 0
        ref[i] = -1
        if f["tid"] == -1:
            n_no_coor += 1
        elif f["tid"] < -1 or f["tid"] >= n_ref or not bc.indexable(r):
            bad[i] = True
        else:
            beg, end = bc.span(r)
            ref[i], bin_[i], wb[i], we[i] = f["tid"], bc.reg2bin(beg, end), beg >> 14, (end - 1) >> 14
        key = bc.sort_key(r, n_ref) if bc.key_ok(r, n_ref) else None       # a record without a key is out of order with nothing
        if first_unsorted < 0 and key is not None and prev_key is not None and key < prev_key:
            first_unsorted = i
        prev_key = key
    where = np.flatnonzero(bad)
    return Columns(ref, bin_, wb, we, unm, bad, (len(where), int(where[0]) if len(where) else -1, first_unsorted, n_no_coor))


def runs(ref, bin_, starts, sizes, n_ref):
    """the maximal stretches of consecutive records with equal (ref, bin), ordered by (refID, bin, file order) with those of ref = -1
    behind every reference -> (chunk_ref, chunk_bin int32, chunk_beg, chunk_end int64): the stream offset of the first record's
    block_size word and the offset behind the last record"""
    ref, bin_ = np.asarray(ref, dtype=np.int32), np.asarray(bin_, dtype=np.int32)
    starts, sizes = np.asarray(starts, dtype=np.int64), np.asarray(sizes, dtype=np.int64)
    n = len(ref)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    head = np.ones(n, bool)
    head[1:] = (ref[1:] != ref[:-1]) | (bin_[1:] != bin_[:-1])
    h = np.flatnonzero(head)
    last = np.append(h[1:], n) - 1
    r, b = ref[h], bin_[h]
    order = np.lexsort((h, b, np.where(r < 0, n_ref, r)))                   # (the last key is the first to count)
    return r[order], b[order], (starts[h] - 4)[order], (starts[last] + sizes[last])[order]


def linear(ref, win_beg, win_end, unmapped, starts, sizes, n_ref):
    """per reference: n_intv = 1 + the largest win_end (0 without records), the records with flag 0x4 clear and set, the first
    record's start and the offset behind the last one (`used` False: no records, the two offsets are undefined and not to be
    compared); and the linear index, lin[lin_off[t] + w] = the smallest start among t's records with win_beg <= w <= win_end, a window
    that no record touches taking the next touched window's value.  Window by window, the plain way."""
    n_intv = np.zeros(n_ref, np.int32)
    n_map, n_un, first, last = (np.zeros(n_ref, np.int64) for _ in range(4))
    used = np.zeros(n_ref, bool)
    wins = [dict() for _ in range(n_ref)]
    for i in range(len(ref)):
        t = int(ref[i])
        if t < 0:
            continue
        beg, end = int(starts[i]) - 4, int(starts[i]) + int(sizes[i])
        if not used[t]:
            used[t], first[t], last[t] = True, beg, end
        first[t], last[t] = min(first[t], beg), max(last[t], end)
        n_intv[t] = max(n_intv[t], int(win_end[i]) + 1)
        if unmapped[i]:
            n_un[t] += 1
        else:
            n_map[t] += 1
        for w in range(int(win_beg[i]), int(win_end[i]) + 1):
            if w not in wins[t] or beg < wins[t][w]:
                wins[t][w] = beg
    lin_off = np.concatenate(([0], np.cumsum(n_intv, dtype=np.int64))).astype(np.int64)
    lin = np.zeros(int(lin_off[-1]), np.int64)
    for t in range(n_ref):
        nxt = None
        for w in range(int(n_intv[t]) - 1, -1, -1):
            nxt = wins[t].get(w, nxt)
            assert nxt is not None                                          # (the last window is some record's win_end)
            lin[lin_off[t] + w] = nxt
    return Linear(n_intv, n_map, n_un, first, last, used, lin_off, lin)


def voffsets(u, member_u, member_c):
    """c_m << 16 | (u - u_m) for the LAST member entry with u_m <= u; anything outside [u_0, u_last] gives 2^64 - 1"""
    mu, mc = [int(v) for v in member_u], [int(v) for v in member_c]
    out = []
    for v in (int(x) for x in u):
        if v < mu[0] or v > mu[-1]:
            out.append(NONE)
        else:
            m = bisect_right(mu, v) - 1
            out.append(mc[m] << 16 | (v - mu[m]))
    return np.array(out, dtype=np.uint64)


def bai_bytes(n_ref, chunks, n_intv, n_mapped, n_unmapped, first, last, lin_off, lin, n_no_coor, voff):
    """the arrays as the bytes of a .bai (SAM specification 5.2): per reference its bins in the order of `chunks` (chunk_ref, chunk_bin,
    chunk_beg, chunk_end as runs() orders them), one chunk list per bin, the pseudo-bin 37450 last, then the linear index; n_no_coor
    behind the references.  voff: stream offsets (int64 array) -> virtual offsets."""
    c_ref, c_bin, c_beg, c_end = chunks
    nc = len(c_ref)
    vb, ve = (voff(np.asarray(a, dtype=np.int64)) if nc else [] for a in (c_beg, c_end))
    vl = voff(np.asarray(lin, dtype=np.int64)) if len(lin) else []
    used = sorted({int(t) for t in c_ref if t >= 0})                         # (first / last of the others are undefined: never looked at)
    at = {t: k for k, t in enumerate(used)}
    vf, vz = (voff(np.asarray(a, dtype=np.int64)[used]) if used else [] for a in (first, last))
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    c = 0
    for t in range(n_ref):
        e = c
        while e < nc and c_ref[e] == t:
            e += 1
        if e == c:                                                          # a reference without records
            out.append(struct.pack("<ii", 0, 0))
            continue
        out.append(struct.pack("<i", 1 + len({int(b) for b in c_bin[c:e]})))
        while c < e:
            g = c
            while g < e and c_bin[g] == c_bin[c]:
                g += 1
            out.append(struct.pack("<Ii", int(c_bin[c]), g - c))
            out += [struct.pack("<QQ", int(vb[k]), int(ve[k])) for k in range(c, g)]
            c = g
        out.append(struct.pack("<IiQQQQ", PSEUDO_BIN, 2, int(vf[at[t]]), int(vz[at[t]]), int(n_mapped[t]), int(n_unmapped[t])))
        out.append(struct.pack("<i", int(n_intv[t])))
        out += [struct.pack("<Q", int(vl[w])) for w in range(int(lin_off[t]), int(lin_off[t + 1]))]
    out.append(struct.pack("<Q", n_no_coor))
    return b"".join(out)


def reference_bai(recs, n_ref, first, voff):
    """the .bai of the sorted records `recs` laid out from stream offset `first`, all of it by this module"""
    starts, sizes = starts_and_sizes(recs, first)
    col = columns(recs, n_ref)
    assert col.status[:3] == (0, -1, -1), col.status
    ln = linear(col.ref, col.win_beg, col.win_end, col.unmapped, starts, sizes, n_ref)
    return bai_bytes(n_ref, runs(col.ref, col.bin, starts, sizes, n_ref), ln.n_intv, ln.n_mapped, ln.n_unmapped, ln.first, ln.last, ln.lin_off, ln.lin,
                     col.status[3], voff)
