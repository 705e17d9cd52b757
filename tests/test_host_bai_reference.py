"""The reference of tests/bai_cases.py, which judges the index kernels at the ABI (tests/test_gpu_bai_abi.py), pinned to statements
that were there before it: the .bai it lays out must answer region queries exactly through the spec-derived reader of
tests/bai_reader.py, on a zlib-written BAM and with no device anywhere; its vectorised `runs` must equal a per-record loop."""
import random

import numpy as np

from tests import bai_cases as bai
from tests import bam_sort_cases as bc
from tests import gz_util
from tests.bai_reader import IndexedBam
from tests.tabix_reader import bgzf_members
from tests.test_host_bam_spec import header, record

TARGETS = [("a", 1 << 29), ("b", 5000), ("c", 300000), ("d", 70000), ("e", 40)]


def edge_records():
    """the hand-made records of tests/test_gpu_bamsort_cli.py's main_records, on these targets"""
    end = 1 << 29
    return [record("at_the_end", 0, 0, end - 100, 60, "100M"), record("big_start", 16, 0, 0, 60, "30M"), record("big_mid", 0, 0, 1 << 28, 60, "10M5000N10M"),
            bc.cg_record("cg_long", 0, 2, 150000, "5S" + "2M1D" * 300 + "20M"), record("mate_unmapped", 4 | 1 | 64, 2, 16384, 0, "", l_seq=20, mtid=2, mpos=16384),
            record("window_edge", 0, 2, 16383, 60, "2M"), record("window_edge2", 0, 2, 32768, 60, "1M")]


def member_table(blob, stream_bytes):
    """stream offset and file offset of every member of a BGZF file, the EOF member standing for the stream's end"""
    mu, mc, acc = [], [], 0
    for off, data in bgzf_members(blob):
        mu.append(acc)
        mc.append(off)
        acc += len(data)
    assert acc == stream_bytes == mu[-1]
    return mu, mc


def test_region_queries_on_the_references_own_bai(tmp_path):
    rng = random.Random(41)
    recs = bc.sorted_records(bc.random_records(rng, 2500, TARGETS, unplaced=0.04) + edge_records(), len(TARGETS))
    head = header(TARGETS)
    stream = head + b"".join(recs)
    blob = gz_util.bgzf(stream, block=30011)                                # (members cut anywhere; several of them)
    mu, mc = member_table(blob, len(stream))
    assert len(mu) > 5
    bam = tmp_path / "ref.bam"
    bam.write_bytes(blob)
    (tmp_path / "ref.bam.bai").write_bytes(bai.reference_bai(recs, len(TARGETS), len(head), lambda u: bai.voffsets(u, mu, mc)))
    ib = IndexedBam(bam)
    assert [r for _, r in ib.records] == recs and ib.targets == TARGETS
    assert ib.bai["n_no_coor"] == sum(1 for r in recs if bc.fields(r)["tid"] < 0) > 0
    regions = []
    for _ in range(300):
        tid = rng.choice((0, 0, 1, 2, 2, 2, 3, 4))
        tlen = TARGETS[tid][1]
        beg = rng.randrange(tlen)
        regions.append((tid, beg, min(tlen, beg + rng.choice((1, 10, 1000, 20000, 200000, tlen)))))
    for tid in (2, 3):
        for edge in range(16384, TARGETS[tid][1], 16384):
            regions += [(tid, edge - 1, edge), (tid, edge, edge + 1), (tid, edge - 1, edge + 1)]
    end = 1 << 29
    regions += [(0, end - 1, end), (0, end - 100, end - 99), (0, end - 101, end - 100), (0, 0, end), (0, (1 << 28) + 2000, (1 << 28) + 2001), (2, 0, 300000),
                (2, 150000 + 919, 150000 + 920), (2, 150000 + 920, 150000 + 921), (4, 0, 40), (4, 39, 40), (1, 0, 1)]
    hits = 0
    for tid, beg, e in regions:
        want = ib.brute(tid, beg, e)
        assert ib.fetch(tid, beg, e) == want, (tid, beg, e)
        assert ib.fetch(tid, beg, e, use_linear=False) == want, (tid, beg, e)
        hits += len(want)
    assert hits > 1000


def test_vectorised_runs_equal_a_plain_loop():
    rng = random.Random(42)
    n, n_ref = 5000, 6
    ref = np.array(sorted(rng.choice((0, 1, 1, 3, 5)) for _ in range(n - 300)) + [-1] * 300, dtype=np.int32)
    bin_ = np.array([0 if r < 0 else rng.choice((0, 1, 9, 4681, 4682)) for r in ref], dtype=np.int32)
    sizes = np.array([rng.randrange(32, 400) for _ in range(n)], dtype=np.int64)
    starts = 101 + 4 + np.concatenate(([0], np.cumsum(sizes + 4)[:-1]))
    plain = []                                                              # [sort ref, bin, first ordinal, beg, end]
    for i in range(n):
        if i and ref[i] == ref[i - 1] and bin_[i] == bin_[i - 1]:
            plain[-1][4] = int(starts[i] + sizes[i])
        else:
            plain.append([n_ref if ref[i] < 0 else int(ref[i]), int(bin_[i]), i, int(starts[i]) - 4, int(starts[i] + sizes[i])])
    plain.sort()
    got = bai.runs(ref, bin_, starts, sizes, n_ref)
    assert len(plain) > 2000 and plain[-1][0] == n_ref and len({(p[0], p[1]) for p in plain}) < len(plain)
    assert [g.tolist() for g in got] == [[-1 if p[0] == n_ref else p[0] for p in plain], [p[1] for p in plain], [p[3] for p in plain], [p[4] for p in plain]]
