#!/usr/bin/env python3
"""Generate tests/golden/corrected_dup_cases.npz by RUNNING the reference's share/palace/scripts/corrected_dup.py on the seeded cases
of tests/corrected_dup_cases.golden_inputs().  The script imports pyfaidx and Biopython, which are absent here and which the code it
runs never calls: a one-line `pyfaidx` module and tests/golden/bio_standin are put on PYTHONPATH.  Its `samtools depth -r <contig>
<bam>` calls are answered by a stand-in `samtools` written into a temporary directory at the head of PATH: it reads the case's
per-contig table (the file handed over as the BAM: name, sum, covered), exits 1 for a contig the table lacks, prints nothing for one
without coverage, and otherwise `covered` positions whose depths sum to `sum`.  So the file PINS what the script does with the depths
and the paths, and does NOT pin samtools.
Every case runs under PYTHONHASHSEED 0, 1, 2 and 3 and is stored only when the four runs exit 0 with the same bytes; the others are
counted.  Asserted: at most a tenth of the cases is left out, and at least half of the stored ones wrote a line that is no input line.
Build-container only; stored per case: the inputs, the depth table, min_len, the output bytes and stdout -- no reference source text."""
import os
import stat
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import corrected_dup_cases as cd  # noqa: E402

REF = "/root/reference/share/palace/scripts/corrected_dup.py"
STANDIN = os.path.join(ROOT, "tests", "golden", "bio_standin")

SAMTOOLS = """#!{python}
import sys
if sys.argv[1:3] != ["depth", "-r"] or len(sys.argv) != 5:
    sys.exit(2)
table = {{}}
for row in open(sys.argv[4]).read().splitlines():
    name, total, covered = row.split("\\t")
    table[name] = (int(total), int(covered))
if sys.argv[3] not in table:
    sys.exit(1)
total, covered = table[sys.argv[3]]
for k in range(covered):
    print(sys.argv[3], k + 1, total // covered + (1 if k < total % covered else 0), sep="\\t")
"""


def u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def main():
    blob, left_out, rewritten = {}, [], 0
    with tempfile.TemporaryDirectory(prefix="palace_corrected_dup_") as top:
        tools = os.path.join(top, "tools")
        os.mkdir(tools)
        open(os.path.join(tools, "pyfaidx.py"), "w").write("Fasta = None\n")
        sam = os.path.join(tools, "samtools")
        open(sam, "w").write(SAMTOOLS.format(python=sys.executable))
        os.chmod(sam, os.stat(sam).st_mode | stat.S_IXUSR)
        cases = cd.golden_inputs()
        for name, case in cases.items():
            d = os.path.join(top, name)
            os.mkdir(d)
            for fn, key in (("edges.fasta.fai", "fai"), ("cycle.txt", "cycle"), ("final_all.txt", "final"), ("before_cut.txt", "before_cut"), ("depth.bam", "depth")):
                open(os.path.join(d, fn), "wb").write(case[key])
            runs = []
            for seed in range(4):
                env = dict(os.environ, PYTHONPATH=tools + os.pathsep + STANDIN, PATH=tools + os.pathsep + os.environ["PATH"], PYTHONHASHSEED=str(seed))
                out = os.path.join(d, f"out{seed}")
                p = subprocess.run([sys.executable, REF, out, "prefix", "cycle.txt", "final_all.txt", "final.txt", "final.fasta", "edges.fasta", "cycle_nodup.txt",
                                    "depth.bam", "before_cut.txt", str(case["min_len"])], cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                runs.append((p.returncode, open(os.path.join(out, "final.txt"), "rb").read() if p.returncode == 0 else p.stderr[-300:], p.stdout,
                             os.path.getsize(os.path.join(out, "cycle_nodup.txt")) if p.returncode == 0 else -1))
            if any(r != runs[0] for r in runs) or runs[0][0] != 0 or runs[0][3] != 0:
                left_out.append((name, [r[0] for r in runs]))
                continue
            for key in ("fai", "cycle", "final", "before_cut", "depth"):
                blob[f"{name}__{key}"] = u8(case[key])
            blob[name + "__min_len"] = np.array([case["min_len"]], np.int64)
            blob[name + "__out"], blob[name + "__stdout"] = u8(runs[0][1]), u8(runs[0][2])
            given = set(case["cycle"].splitlines()) | set(case["final"].splitlines())
            rewritten += any(row not in given for row in runs[0][1].splitlines())
    stored = len(cases) - len(left_out)
    print("left out:", left_out)
    print(f"{len(cases)} cases, {stored} stored, {rewritten} with a rewritten line")
    assert len(cases) >= 60 and 10 * len(left_out) <= len(cases) and 2 * rewritten >= stored
    path = os.path.join(ROOT, "tests", "golden", "corrected_dup_cases.npz")
    np.savez_compressed(path, **blob)
    print(os.path.getsize(path))


if __name__ == "__main__":
    main()
