#!/usr/bin/env python3
"""Split a FASTG into the FASTA of its nodes.

Counterpart of the reference's share/palace/scripts/split_fastg.py (call site palace:389-397): the same command line
    split_fastg.py -g <assembly_graph.fastg> [-o <assembly_graph.fasta>]
and, with --fai, the two index files of the `samtools faidx` runs behind it (palace:399-406).  The work is bin/split_fastg's (the
FASTG indexed, its records named and the FASTA gathered on the GPU; the rules: DESIGN.md 8): this file starts it as a child process
and passes its stdout, stderr and exit status on.  There is no Python implementation behind it -- without the executable or a
device the step fails.
Parity status: PINNED for texts inside the grammar of DESIGN.md 8 -- tests/golden/split_fastg_cases.npz holds what the reference's
script wrote; texts outside it are declined (exit 1), and the `.fai` rows are the documented five columns (samtools is absent).
"""
import os
import subprocess
import sys

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "split_fastg")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(BINARY):
        print(f"split_fastg.py: {BINARY} is missing (build the host executables first); there is no Python path", file=sys.stderr)
        return 1
    sys.stdout.flush()
    return subprocess.run([BINARY] + list(argv)).returncode


if __name__ == "__main__":
    sys.exit(main())
