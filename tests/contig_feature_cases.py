"""The rules of the phage scorer's input (`phage_scoring`) restated in numpy, the seeded sequences of the golden
file, and the FASTA texts the kernel tests aim at palace_contig_features.  Not a test module."""
import numpy as np

CELLS, FSUMS = 12288, 64
ALPHABET = b"ACGTacgtNnRY-*"
GOLDEN_LENGTHS = (1, 2, 3, 5, 6, 7, 8, 9, 10, 17, 33, 64, 100, 257, 500, 999, 1500, 2048, 2500, 3333, 4095, 4096, 4097, 5000)

_CODE = np.full(256, -1, np.int64)
for _k, _b in enumerate(b"ACGT"):
    _CODE[_b] = _k
    _CODE[_b + 32] = _k                                 # lower case: the reference upper-cases first


def golden_sequences():
    """the inputs of tests/golden/contig_features_cases.npz: none has a digit, none is empty"""
    rng = np.random.default_rng(20240611)
    alphabet = np.frombuffer(ALPHABET, np.uint8)
    return [alphabet[rng.integers(0, len(alphabet), size=n)].tobytes() for n in GOLDEN_LENGTHS]


def counts(seq: bytes):
    """(C[3, 64, 64] int64, m): every byte but A C G T a c g t is dropped BEFORE the 3-mers are formed"""
    v = _CODE[np.frombuffer(seq, np.uint8)]
    v = v[v >= 0]
    m = len(v)
    c = np.zeros((3, 64, 64), np.int64)
    if m >= 3:
        loc = 16 * v[:-2] + 4 * v[1:-1] + v[2:]
        for d in range(3):
            k = m - 5 - d
            if k > 0:
                np.add.at(c[d], (loc[:k], loc[3 + d:3 + d + k]), 1)
    return c, m


def reference_features(seq: bytes) -> np.ndarray:
    """what encode.matrix_encoding(seq, 3) returns: float64[12288], cell (d, a, b) at d * 4096 + a * 64 + b"""
    c, _ = counts(seq)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c.reshape(-1).astype(np.float64) / np.float64(len(seq)) * 100


def model_features(seq: bytes):
    """(feat float32[12288] with cell (d, a, b) at (a * 64 + b) * 3 + d, fsum float32[64] from the exact integer row sums)"""
    c, _ = counts(seq)
    with np.errstate(invalid="ignore", divide="ignore"):
        feat = (np.moveaxis(c, 0, 2).reshape(-1).astype(np.float64) / np.float64(len(seq)) * 100).astype(np.float32)
        fsum = (c[0].sum(axis=1).astype(np.float64) / np.float64(len(seq)) * 100).astype(np.float32)
    return feat, fsum


def reference_fsum(feat64: np.ndarray) -> np.ndarray:
    """the reference's source-node input: 64 doubles summed, then rounded to float32"""
    return np.sum(feat64.reshape(3, 64, 64)[0], axis=1).astype(np.float32)


def fasta(records, width=60, crlf=False, final_lf=True):
    """(text, for each record the text offsets of its sequence bytes): records are (name, sequence) pairs"""
    end = b"\r\n" if crlf else b"\n"
    parts, offsets, at = [], [], 0
    for name, seq in records:
        head = b">" + name + end
        parts.append(head)
        at += len(head)
        offs = np.empty(len(seq), np.int64)
        for lo in range(0, len(seq), width):
            line = seq[lo:lo + width]
            offs[lo:lo + len(line)] = np.arange(at, at + len(line))
            parts.append(line + end)
            at += len(line) + len(end)
        offsets.append(offs)
    text = b"".join(parts)
    if not final_lf and text.endswith(end):
        text = text[:len(text) - len(end)]
    return text, offsets


def first_digit(records, offsets, r0, r1) -> int:
    """the smallest text offset of a byte 0-9 in a sequence of records [r0, r1), else -1"""
    best = -1
    for (_, seq), offs in zip(records[r0:r1], offsets[r0:r1]):
        a = np.frombuffer(seq, np.uint8)
        hit = np.flatnonzero((a >= 48) & (a <= 57))
        if hit.size and (best < 0 or offs[hit[0]] < best):
            best = int(offs[hit[0]])
    return best


def dna(rng, n, alphabet=b"ACGT") -> bytes:
    a = np.frombuffer(alphabet, np.uint8)
    return a[rng.integers(0, len(a), size=n)].tobytes()


def kernel_cases(rng, chunk):
    """name -> (records, keyword arguments of fasta()): the inputs the kernel test names one by one"""
    cases = {}
    small = [(b"m%d" % m, dna(rng, m)) for m in range(10)]
    cases["m_0_to_9"] = (small, {})
    cases["odd_records"] = ([(b"onlyN", b"N" * 50), (b"len1", b"G"), (b"len0", b""), (b"after", dna(rng, 30)),
                             (b"inside_3mer", b"ACNGTTNNACG-TACGT*ACGGTCA"), (b"in_gap", b"ACGTTNNNNNNNNNNACGTACGTAC"),
                             (b"lower", dna(rng, 200, b"acgt")), (b"mixed", dna(rng, 500, ALPHABET))], {})
    for width in (1, 7, 60, 64):
        cases["width_%d" % width] = ([(b"a", dna(rng, 333, ALPHABET)), (b"b", dna(rng, 64)), (b"c", dna(rng, 129, ALPHABET))], {"width": width})
    cases["crlf"] = ([(b"a", dna(rng, 250, ALPHABET)), (b"b", dna(rng, 61))], {"crlf": True})
    cases["no_final_lf"] = ([(b"a", dna(rng, 100)), (b"last", dna(rng, 75, ALPHABET))], {"final_lf": False})
    cases["crosses_tile"] = ([(b"lead", dna(rng, 3900)), (b"across", dna(rng, 600, ALPHABET)), (b"tail", dna(rng, 10))], {})
    # the chunk constant counts positions of S, kept or dropped: both the length and the compact length walk across it
    border = []
    for delta in range(-8, 9):
        border.append((b"len%+d" % delta, dna(rng, chunk + delta, ALPHABET)))
        kept = dna(rng, chunk + delta)
        border.append((b"kept%+d" % delta, kept[:1000] + b"N" * 37 + kept[1000:]))
    cases["chunk_border"] = (border, {})
    cases["two_chunks_exact"] = ([(b"x", dna(rng, 2 * chunk)), (b"y", dna(rng, 2 * chunk + 1, ALPHABET)), (b"z", b"N" * chunk + dna(rng, 7)),
                                 (b"halo", dna(rng, chunk - 3) + b"N" * 40 + dna(rng, 5))], {})
    cases["poly_a_70000"] = ([(b"polyA", b"A" * 70000)], {})
    cases["many_short"] = ([(b"s%d" % k, dna(rng, int(n), ALPHABET)) for k, n in enumerate(rng.integers(1, 41, size=3000))], {})
    cases["long_between_short"] = ([(b"s0", dna(rng, 20)), (b"long", dna(rng, 300000, ALPHABET)), (b"s1", dna(rng, 45)), (b"s2", b"")], {})
    return cases
