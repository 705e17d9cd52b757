#!/usr/bin/env python3
"""Test every path for a (fuzzy) cycle, trim the cycles and write the final FASTA.

Counterpart of the reference's share/palace/scripts/make_final_fa.py (call site palace:877-882): the same command line
    make_final_fa.py <final.txt> <filtered_graph.txt> <assembly_graph.fasta> <final.fasta> <prefix>
                     [--trim_threshold N] [--min_cycle_length N]
without the Biopython dependency.  The work is bin/make_final_fa's (node ids, the cycle test, the FASTA's index and the output
text on the GPU; the rules and the declared deviations: DESIGN.md 8): this file starts it as a child process and passes its
stdout, stderr and exit status on.  There is no Python implementation behind it -- without the executable or a device the step
fails.
Parity status: the graph rules, the cycle decision, the order, the numbering, the separators and the headers are PINNED by
tests/golden/final_fa_cases.npz (the reference script itself, run over a stand-in for the two Biopython calls it makes); the
FASTA reader and the complement table are UNPINNED -- Biopython is absent where the golden file is made.
"""
import os
import subprocess
import sys

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "make_final_fa")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(BINARY):
        print(f"make_final_fa.py: {BINARY} is missing (build the host executables first); there is no Python path", file=sys.stderr)
        return 1
    sys.stdout.flush()
    return subprocess.run([BINARY] + list(argv)).returncode


if __name__ == "__main__":
    sys.exit(main())
