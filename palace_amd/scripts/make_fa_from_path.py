#!/usr/bin/env python3
"""Write the sequences of matching's paths as FASTA.

Counterpart of the reference's share/palace/scripts/make_fa_from_path.py (call sites palace:697-700, 747-750, 778-781;
SURVEY.md "next" row N5): the same command line
    make_fa_from_path.py <assembly.fasta> <paths> <out.fasta> <mode>
without the pysam dependency.  The work is bin/make_fa_from_path's (the FASTA indexed and the output gathered on the GPU; the
rules: DESIGN.md 8): this file starts it as a child process and passes its stdout, stderr and exit status on.  There is no
Python implementation behind it -- without the executable or a device the step fails.
Parity status: UNPINNED -- the reference script cannot run here (pysam is absent); tests hold a restatement of the rules.
"""
import os
import subprocess
import sys

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "make_fa_from_path")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(BINARY):
        print(f"make_fa_from_path.py: {BINARY} is missing (build the host executables first); there is no Python path", file=sys.stderr)
        return 1
    sys.stdout.flush()
    return subprocess.run([BINARY] + list(argv)).returncode


if __name__ == "__main__":
    sys.exit(main())
