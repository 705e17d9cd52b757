"""A stand-in of our own for the two Biopython calls the reference's make_final_fa.py makes, used by
tests/golden/make_final_fa_golden.py on the machine that makes the golden file and nowhere else: `SeqIO.parse(path, "fasta")` with
`SeqIO.to_dict`, and `Seq` with `+` and `reverse_complement`.  It is not Biopython and pins nothing about Biopython: the FASTA
reader and the complement table of the golden outputs are this package's (UNPINNED)."""
