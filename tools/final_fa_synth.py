#!/usr/bin/env python3
"""A graph file for timing make_final_fa on the synthetic assembly of tools/path_fasta_synth.py (profiles/make_final_fa.md; CPU).

    python tools/final_fa_synth.py <dir>

reads <dir>/paths.txt (tokens `<contig><strand>`, TAB-separated) and writes <dir>/graph.txt: per path one JUNC line -- for an even
path the arc last token -> first token, which closes the whole path, for an odd one the arc third token -> second token, which
closes an interval that trims both ends -- between SEG lines, which make_final_fa passes over."""
import os
import sys


def main():
    d = sys.argv[1]
    n = 0
    with open(os.path.join(d, "paths.txt"), "rb") as f, open(os.path.join(d, "graph.txt"), "wb") as g:
        for k, line in enumerate(f):
            t = line.split()
            if not t:
                continue
            a, b = (t[-1], t[0]) if k % 2 == 0 or len(t) < 4 else (t[2], t[1])
            g.write(b"SEG %s 17 1\nJUNC %s %s %s %s 12 0 0\n" % (t[0][:-1], a[:-1], a[-1:], b[:-1], b[-1:]))
            n += 1
    print(f"{n} JUNC lines")


if __name__ == "__main__":
    main()
