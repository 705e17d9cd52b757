#!/usr/bin/env python3
"""Generate tests/golden/final_fa_cases.npz by RUNNING the reference's share/palace/scripts/make_final_fa.py on the seeded inputs
of tests/final_fa_cases.golden_inputs(), every one of them inside the grammar of DESIGN.md 8.  The script imports Biopython, which
is absent here: tests/golden/bio_standin (a package `Bio` of our own with the two calls the script makes) is put on PYTHONPATH.
So the file PINS what the script itself does -- the graph rules, the cycle decision, the order, the numbering, the separators, the
headers, the stderr lines -- and does NOT pin Biopython's FASTA reader or its complement table.
Build-container only; the GPU box reads the committed .npz.  Stored: the inputs, the option words, the output bytes and stderr (the
script runs in the case's directory with relative file names, so stderr names `asm.fasta` and `out.fasta`) -- no reference source
text.  The reference must exit 0 with an empty stdout on every stored case."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import final_fa_cases as fc  # noqa: E402

REF = "/root/reference/share/palace/scripts/make_final_fa.py"
STANDIN = os.path.join(ROOT, "tests", "golden", "bio_standin")


def u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def main():
    blob = {}
    env = dict(os.environ, PYTHONPATH=STANDIN)
    with tempfile.TemporaryDirectory(prefix="palace_final_fa_") as top:
        for name, (paths, graph, fasta, prefix, words) in fc.golden_inputs().items():
            d = os.path.join(top, name)
            os.mkdir(d)
            for fn, text in (("final.txt", paths), ("graph.txt", graph), ("asm.fasta", fasta)):
                open(os.path.join(d, fn), "wb").write(text)
            p = subprocess.run([sys.executable, REF, "final.txt", "graph.txt", "asm.fasta", "out.fasta", prefix.decode()] + [w.decode() for w in words],
                               cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0 and p.stdout == b"", (name, p.returncode, p.stderr[-600:])
            blob[name + "__paths"], blob[name + "__graph"], blob[name + "__fasta"] = u8(paths), u8(graph), u8(fasta)
            blob[name + "__prefix"], blob[name + "__args"] = u8(prefix), u8(b"\0".join(words))
            blob[name + "__out"] = u8(open(os.path.join(d, "out.fasta"), "rb").read())
            blob[name + "__err"] = u8(p.stderr)
    path = os.path.join(ROOT, "tests", "golden", "final_fa_cases.npz")
    np.savez_compressed(path, **blob)
    print({k: len(v) for k, v in blob.items() if k.endswith(("__out", "__err"))}, os.path.getsize(path))


if __name__ == "__main__":
    main()
