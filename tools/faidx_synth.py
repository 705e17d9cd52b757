#!/usr/bin/env python3
"""A synthetic assembly FASTA and a region file for the traced runs of faidx (profiles/faidx.md; CPU, numpy only).

    python tools/faidx_synth.py <out dir> [--contigs N] [--regions M]

writes <out dir>/assembly.fasta -- N contigs (default 4 000) of 200 to 4 999 bases named NODE_<i>_length_<n>_cov_<c>, folded at 60
bases -- and <out dir>/regions.txt -- M regions (default 120 000), three in four `name:B-E` of at most 1 200 bases at a random place,
one in four a whole contig."""
import argparse
import os

import numpy as np

ALPHABET = np.frombuffer(b"ACGTacgtNnRy*", dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--contigs", type=int, default=4000)
    ap.add_argument("--regions", type=int, default=120_000)
    a = ap.parse_args()
    rng = np.random.default_rng(2026)
    lens = rng.integers(200, 5000, size=a.contigs)
    names, out = [], []
    for i, n in enumerate(lens):
        names.append(b"NODE_%d_length_%d_cov_%d" % (i + 1, n, n % 97))
        seq = ALPHABET[rng.integers(0, len(ALPHABET), size=int(n))].tobytes()
        out.append(b">" + names[-1] + b"\n" + b"".join(seq[k:k + 60] + b"\n" for k in range(0, len(seq), 60)))
    os.makedirs(a.out_dir, exist_ok=True)
    text = b"".join(out)
    with open(os.path.join(a.out_dir, "assembly.fasta"), "wb") as f:
        f.write(text)
    regs = []
    for i in rng.integers(0, a.contigs, size=a.regions):
        n = int(lens[i])
        b = int(rng.integers(1, n + 1))
        e = min(n, b + int(rng.integers(0, 1200)))
        regs.append(names[i] + (b":%d-%d" % (b, e) if i % 4 else b""))
    with open(os.path.join(a.out_dir, "regions.txt"), "wb") as f:
        f.write(b"\n".join(regs) + b"\n")
    print(f"{a.contigs} contigs, {int(lens.sum())} bases, assembly.fasta {len(text)} bytes; {a.regions} regions")


if __name__ == "__main__":
    main()
