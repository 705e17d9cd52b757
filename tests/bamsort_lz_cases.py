"""The inputs of the `--lz` tests of `bamsort` and `samview` (tests/test_gpu_bamsort_lz_cli.py), built as the fixtures of
tests/test_gpu_bamsort_cli.py and tests/test_gpu_samview_cli.py are: a BAM of a few thousand records and a SAM text of 3000 lines, and
the streams the tools must write for them by the Python restatements.  tests/test_host_deflate_lz.py holds the exact model of the hashed
matcher to the condition of the flag's being on these streams, without a device.  Test infrastructure."""
import functools
import random

import numpy as np

from tests import bam_sort_cases as bc
from tests import sam_cases as sc
from tests.test_host_bam_spec import header

MEMBER = 0xff00
TARGETS = [("c0", 300000), ("c1", 5000), ("c2", 70000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@PG\tID:aligner\n"


@functools.lru_cache(maxsize=None)
def bam_case():
    """(the input stream, the stream bamsort must write)"""
    recs = bc.random_records(random.Random(1951), 3000, TARGETS, unplaced=0.03)
    return header(TARGETS, TEXT) + b"".join(recs), header(TARGETS, bc.rewrite_text(TEXT)) + b"".join(bc.sorted_records(recs, len(TARGETS)))


@functools.lru_cache(maxsize=None)
def sam_case():
    """(the SAM text, the stream samview -F 0x800 must write)"""
    rng = np.random.default_rng(1952)
    lines = []
    for _ in range(3000):
        f = sc.valid_line(rng).split(b"\t")
        f[3] = b"%d" % int(rng.integers(0, 800))                             # (a place a .bai can hold)
        lines.append(b"\t".join(f))
    text = sc.HEADER + b"\n".join(lines) + b"\n"
    recs, _, first = sc.text_verdict(text, 0x800)
    assert first is None
    return text, sc.bam_header(text) + b"".join(recs)


def pieces(stream):
    return [stream[at:at + MEMBER] for at in range(0, len(stream), MEMBER)]
