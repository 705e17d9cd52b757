#!/usr/bin/env python3
"""A synthetic assembly for timing make_fa_from_path (profiles/path_fasta.md; CPU, numpy only).

    python tools/path_fasta_synth.py <out dir> [--contigs N] [--per-path K] [--width W]

writes <out dir>/assembly.fasta -- N contigs (default 1 000 000) with the length law and the names of the 1M-contig bench sample
(bench/sample.py contig_lengths, palace_amd/synth.py contig_names: log-normal, median 800, sigma 1, at least 56 bases; about 1.3 GB),
folded at W bases (default 60) -- and <out dir>/paths.txt, which names every contig exactly once in random order, every second one
reversed, K tokens per line (default 4)."""
import argparse
import os

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--contigs", type=int, default=1_000_000)
    ap.add_argument("--per-path", type=int, default=4)
    ap.add_argument("--width", type=int, default=60)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(20240607))
    n, w = a.contigs, a.width
    lens = np.maximum(56, rng.lognormal(np.log(800.0), 1.0, size=n)).astype(np.int64)
    ids = rng.permutation(np.arange(1, 4 * n + 1))[:n]
    covs = rng.gamma(2.0, 8.0, size=n)
    names = [b"EDGE_%d_length_%d_cov_%.6f" % (int(i), int(l), c) for i, l, c in zip(ids, lens, covs)]
    os.makedirs(a.out_dir, exist_ok=True)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    total = 0
    with open(os.path.join(a.out_dir, "assembly.fasta"), "wb") as f:
        for c0 in range(0, n, 20000):                               # a chunk of contigs: its text is laid out with index arithmetic
            ls = lens[c0:c0 + 20000]
            hs = np.array([len(nm) + 2 for nm in names[c0:c0 + len(ls)]], np.int64)          # '>' name LF
            body = ls + (ls + w - 1) // w                           # bases and the LFs of their lines
            start = np.zeros(len(ls) + 1, np.int64)
            np.cumsum(hs + body, out=start[1:])
            out = np.full(int(start[-1]), 10, np.uint8)             # LF wherever nothing else is written
            for k, nm in enumerate(names[c0:c0 + len(ls)]):
                out[start[k]:start[k] + hs[k] - 1] = np.frombuffer(b">" + nm, np.uint8)
            j = np.arange(int(ls.sum()), dtype=np.int64) - np.repeat(np.cumsum(ls) - ls, ls)  # a base's index in its contig
            out[np.repeat(start[:-1] + hs, ls) + j + j // w] = acgt[rng.integers(0, 4, size=len(j))]
            f.write(out.tobytes())
            total += len(out)
    order = rng.permutation(n)
    with open(os.path.join(a.out_dir, "paths.txt"), "wb") as f:
        for p0 in range(0, n, a.per_path):
            f.write(b"\t".join(names[int(c)] + (b"-" if k & 1 else b"+") for k, c in enumerate(order[p0:p0 + a.per_path], start=p0)) + b"\n")
    print(f"{n} contigs, {int(lens.sum())} bases, assembly.fasta {total} bytes, {(n + a.per_path - 1) // a.per_path} paths")


if __name__ == "__main__":
    main()
