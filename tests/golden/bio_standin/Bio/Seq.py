"""`Seq`: a str with `+` and `reverse_complement` by the table of DESIGN.md 8 (ambiguous DNA, either case)."""

_COMP = str.maketrans("ACGTRYKMBDHVacgtrykmbdhv", "TGCAYRMKVHDBtgcayrmkvhdb")


class Seq(str):
    def __add__(self, other):
        return Seq(str.__add__(self, other))

    def reverse_complement(self):
        return Seq(str.translate(self, _COMP)[::-1])
