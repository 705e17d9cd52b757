#!/usr/bin/env python3
"""Filter stage 04's paths by BLAST groups, gene hits and scores; write the filtered FASTA and the cycle list.

Counterpart of the reference's share/palace/scripts/filter_result.py (call site palace:604-612): the same command line
    filter_result.py <fasta> <all_result.txt> <filtered.fasta> <blast> <blast_ratio> <gene_hit> <node_score> <filtered_cycle.txt>
without the Biopython dependency.  The work is bin/filter_result's (the BLAST table's groups, every path's class, the
first-occurrence rule, the FASTA's index and the output text on the GPU; the rules and the declared deviations: DESIGN.md 8): this
file starts it as a child process and passes its stdout, stderr and exit status on.  There is no Python implementation behind it --
without the executable or a device the step fails.
Parity status: the group rule, the score and hit rules, the classes, the first-occurrence rule, stdout's tagged lines and the cycle
file's lines are PINNED by tests/golden/filter_result_cases.npz (the reference script itself, run over a stand-in for the Biopython
calls it makes); the FASTA reader and the complement table are UNPINNED -- Biopython is absent where the golden file is made.  The
order of the cycle file's lines and the two prints of Python objects are declared deviations.
"""
import os
import subprocess
import sys

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "filter_result")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(BINARY):
        print(f"filter_result.py: {BINARY} is missing (build the host executables first); there is no Python path", file=sys.stderr)
        return 1
    sys.stdout.flush()
    return subprocess.run([BINARY] + list(argv)).returncode


if __name__ == "__main__":
    sys.exit(main())
