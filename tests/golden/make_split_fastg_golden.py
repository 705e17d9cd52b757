#!/usr/bin/env python3
"""Generate tests/golden/split_fastg_cases.npz by RUNNING the reference's share/palace/scripts/split_fastg.py (pure stdlib: re,
argparse, os) on the seeded inputs of tests/split_fastg_cases.golden_inputs(), every one of them inside the grammar of DESIGN.md 8.
Build-container only; the GPU box reads the committed .npz.  Stored: the input texts and the output bytes -- no reference source
text.  The reference must exit 0 on every stored case."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import split_fastg_cases as sc  # noqa: E402

REF = "/root/reference/share/palace/scripts/split_fastg.py"


def main():
    blob = {}
    with tempfile.TemporaryDirectory(prefix="palace_split_fastg_") as d:
        for name, text in sc.golden_inputs().items():
            g, o = os.path.join(d, name + ".fastg"), os.path.join(d, name + ".fasta")
            open(g, "wb").write(text)
            p = subprocess.run([sys.executable, REF, "-g", g, "-o", o], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0 and p.stdout == b"", (name, p.returncode, p.stderr[-400:])
            blob[name + "__in"] = np.frombuffer(text, dtype=np.uint8)
            blob[name + "__out"] = np.frombuffer(open(o, "rb").read(), dtype=np.uint8)
        # the default output name, once
        g = os.path.join(d, "default.fastg")
        open(g, "wb").write(sc.golden_inputs()["three_of_one_name"])
        assert subprocess.run([sys.executable, REF, "--graph", g]).returncode == 0
        assert open(os.path.join(d, "default.nodes.fasta"), "rb").read() == blob["three_of_one_name__out"].tobytes()
    path = os.path.join(ROOT, "tests", "golden", "split_fastg_cases.npz")
    np.savez_compressed(path, **blob)
    print({k: len(v) for k, v in blob.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
