"""`parse(path, "fasta")` and `to_dict(records)`: a record's id is the first word of its header line, its sequence the lines up to
the next header with the white space at their ends removed; a second record of one id makes `to_dict` raise."""
from .Seq import Seq


class SeqRecord:
    def __init__(self, id, seq):
        self.id, self.seq = id, seq


def parse(path, fmt):
    assert fmt == "fasta"
    rec_id, parts = None, []
    with open(path, "r") as f:
        for line in f:
            if line.startswith(">"):
                if rec_id is not None:
                    yield SeqRecord(rec_id, Seq("".join(parts)))
                words = line[1:].split()
                rec_id, parts = (words[0] if words else ""), []
            elif rec_id is not None:
                parts.append(line.strip())
    if rec_id is not None:
        yield SeqRecord(rec_id, Seq("".join(parts)))


def to_dict(records):
    out = {}
    for r in records:
        if r.id in out:
            raise ValueError(f"Duplicate key '{r.id}'")
        out[r.id] = r
    return out
