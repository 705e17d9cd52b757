#!/usr/bin/env python3
"""A synthetic SPAdes-shaped FASTG for timing split_fastg (profiles/split_fastg.md; CPU, numpy only).

    python tools/split_fastg_synth.py <out dir> [--edges N] [--width W]

writes <out dir>/assembly_graph.fastg -- N edges (default 200 000) with the length law and the names of the 1M-contig bench sample
(log-normal, median 800, sigma 1, at least 56 bases), each as its forward record `>NAME:NEXT,PREV';` and its primed record
`>NAME':PREV';` (the reverse complement), folded at W bases (default 60): about 2.7 KB per edge."""
import argparse
import os

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--edges", type=int, default=200_000)
    ap.add_argument("--width", type=int, default=60)
    a = ap.parse_args()
    rng = np.random.Generator(np.random.PCG64(20240608))
    n, w = a.edges, a.width
    lens = np.maximum(56, rng.lognormal(np.log(800.0), 1.0, size=n)).astype(np.int64)
    ids = rng.permutation(np.arange(1, 4 * n + 1))[:n]
    covs = rng.gamma(2.0, 8.0, size=n)
    names = [b"EDGE_%d_length_%d_cov_%.6f" % (int(i), int(l), c) for i, l, c in zip(ids, lens, covs)]
    os.makedirs(a.out_dir, exist_ok=True)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    total = 0
    with open(os.path.join(a.out_dir, "assembly_graph.fastg"), "wb") as f:
        for c0 in range(0, n, 20000):                               # a chunk of edges: its text is laid out with index arithmetic
            ls = np.repeat(lens[c0:c0 + 20000], 2)                  # forward, primed, forward, ...
            heads = []
            for k in range(c0, min(c0 + 20000, n)):
                nxt, prv = names[(k + 1) % n], names[k - 1]
                heads += [b">" + names[k] + b":" + nxt + b"," + prv + b"';", b">" + names[k] + b"':" + prv + b"';"]
            hs = np.array([len(h) + 1 for h in heads], np.int64)    # header LF
            body = ls + (ls + w - 1) // w                           # bases and the LFs of their lines
            start = np.zeros(len(ls) + 1, np.int64)
            np.cumsum(hs + body, out=start[1:])
            out = np.full(int(start[-1]), 10, np.uint8)             # LF wherever nothing else is written
            for k, h in enumerate(heads):
                out[start[k]:start[k] + hs[k] - 1] = np.frombuffer(h, np.uint8)
            first = np.cumsum(ls) - ls                              # a record's first base among the chunk's bases
            j = np.arange(int(ls.sum()), dtype=np.int64) - np.repeat(first, ls)               # a base's index in its record
            code = rng.integers(0, 4, size=len(j)).astype(np.uint8)
            primed = np.repeat(np.arange(len(ls)) & 1, ls).astype(bool)
            src = np.repeat(first - np.where(np.arange(len(ls)) & 1, ls, 0), ls) + np.where(primed, np.repeat(ls, ls) - 1 - j, j)
            code = np.where(primed, 3 - code[src], code)            # the primed record: its forward one read from the end, complemented
            out[np.repeat(start[:-1] + hs, ls) + j + j // w] = acgt[code]
            f.write(out.tobytes())
            total += len(out)
    print(f"{n} edges, {2 * n} records, {int(lens.sum())} bases per strand, assembly_graph.fastg {total} bytes")


if __name__ == "__main__":
    main()
