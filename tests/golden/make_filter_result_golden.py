#!/usr/bin/env python3
"""Generate tests/golden/filter_result_cases.npz by RUNNING the reference's share/palace/scripts/filter_result.py on the seeded
inputs of tests/filter_result_cases.golden_inputs(), every one of them inside the grammar of DESIGN.md 8.  The script imports
Biopython, which is absent here: tests/golden/bio_standin (a package `Bio` of our own with the calls the script makes) is put on
PYTHONPATH.  So the file PINS what the script itself does -- the BLAST groups, the score and hit rules, which paths are written and
which are not, the first-occurrence rule, the tagged lines on stdout, the cycle file's lines -- and does NOT pin Biopython's FASTA
reader or its complement table.  The `.fai` the script reads is written here from the FASTA (name, length).
Build-container only; the GPU box reads the committed .npz.  Stored: the inputs, the argument words, the FASTA bytes, the cycle
file's bytes and stdout -- no reference source text.  The reference must exit 0 on every stored case."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import filter_result_cases as fr  # noqa: E402

REF = "/root/reference/share/palace/scripts/filter_result.py"
STANDIN = os.path.join(ROOT, "tests", "golden", "bio_standin")
WORDS = ["asm.fasta", "all_result.txt", "filtered.fasta", "hits.blast", None, "gene_hit.txt", "node_score.txt", "filtered_cycle.txt"]


def u8(b: bytes):
    return np.frombuffer(b, dtype=np.uint8)


def main():
    blob = {}
    env = dict(os.environ, PYTHONPATH=STANDIN)
    with tempfile.TemporaryDirectory(prefix="palace_filter_result_") as top:
        for name, (fasta, paths, blast, ratio, hits, scores) in fr.golden_inputs().items():
            d = os.path.join(top, name)
            os.mkdir(d)
            fai = b"".join(b"%s\t%d\t0\t0\t0\n" % (k, len(v)) for k, v in fr.parse_fasta(fasta).items())
            for fn, text in (("asm.fasta", fasta), ("asm.fasta.fai", fai), ("all_result.txt", paths), ("hits.blast", blast), ("gene_hit.txt", hits),
                             ("node_score.txt", scores)):
                open(os.path.join(d, fn), "wb").write(text)
            words = [w if w else ratio.decode() for w in WORDS]
            p = subprocess.run([sys.executable, REF] + words, cwd=d, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            assert p.returncode == 0 and p.stderr == b"", (name, p.returncode, p.stderr[-600:])
            for key, val in (("fasta", fasta), ("paths", paths), ("blast", blast), ("hits", hits), ("scores", scores), ("args", "\0".join(words).encode())):
                blob[name + "__" + key] = u8(val)
            blob[name + "__out"] = u8(open(os.path.join(d, "filtered.fasta"), "rb").read())
            blob[name + "__cycle"] = u8(open(os.path.join(d, "filtered_cycle.txt"), "rb").read())
            blob[name + "__stdout"] = u8(p.stdout)
    path = os.path.join(ROOT, "tests", "golden", "filter_result_cases.npz")
    np.savez_compressed(path, **blob)
    print({k: len(v) for k, v in blob.items() if k.endswith(("__out", "__cycle"))}, os.path.getsize(path))


if __name__ == "__main__":
    main()
