#!/usr/bin/env python3
"""Correct the cycles' tandem copies by depth, drop similar paths and write <prefix>_final.txt.

Counterpart of the reference's share/palace/scripts/corrected_dup.py (call site palace:864-875): the same command line
    corrected_dup.py <out_dir> <prefix> <cycle_file> <final_all_file> <final.txt> <final.fasta> <edge_fasta> <cycle_nodup.txt>
                     <bam> <before_cut> <min_len>
without pyfaidx, Biopython, numpy and without a `samtools` on PATH; `--contig-depth <table>` in front hands over the table
`bamdepth --per-contig` printed, and the BAM is then not opened.  The work is bin/corrected_dup's (names, depth per contig, borders,
tandem candidates, the similarity relation and the base-set test on the GPU; the rules and the declared deviations: DESIGN.md 8):
this file starts it as a child process and passes its stdout, stderr and exit status on.  There is no Python implementation behind
it -- without the executable or a device the step fails.
Parity status: the rules are PINNED by tests/golden/corrected_dup_cases.npz (the reference script itself, run over stand-ins for
pyfaidx, Biopython and `samtools depth -r`); samtools' own depth rules are those of palace_depth_per_contig.
"""
import os
import subprocess
import sys

BINARY = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bin", "corrected_dup")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not os.path.exists(BINARY):
        print(f"corrected_dup.py: {BINARY} is missing (build the host executables first); there is no Python path", file=sys.stderr)
        return 1
    sys.stdout.flush()
    return subprocess.run([BINARY] + list(argv)).returncode


if __name__ == "__main__":
    sys.exit(main())
