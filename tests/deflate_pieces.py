"""Inputs of the BGZF writer's tests (palace_bgzf_deflate on the device, csrc/deflate_enc.hpp on a CPU): the pieces whose members
must inflate to themselves, and depth-like text for the size comparison with zlib.  Test infrastructure."""
import numpy as np

MAX_TEXT = 0xff00


def depth_lines(name, positions, depths):
    return b"".join(b"%s\t%d\t%d\n" % (name, p, d) for p, d in zip(positions, depths))


def fibonacci_piece():
    """22 distinct byte values with frequencies 1, 1, 2, 3, ... 17 711 (46 367 bytes, no newline): an unrestricted Huffman tree
    of the bytes alone is 21 levels deep.  (With the end-of-block code as a third 1, ties let an optimal tree be 12 levels deep:
    tests/deflate_enc_cases.py has the piece that forces the length limit.)"""
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    assert fib[-1] == 17711 and sum(fib) == 46367
    vals = [v for v in range(65, 65 + 22)]
    raw = np.concatenate([np.full(f, v, np.uint8) for f, v in zip(fib, vals)])
    np.random.default_rng(20240).shuffle(raw)
    assert 10 not in set(vals)
    return raw.tobytes()


def pieces():
    """[(name, bytes)], every one at most 0xff00 bytes"""
    rng = np.random.default_rng(77)
    name = b"NODE_17_length_2964_cov_12.31"
    rolls = b"".join(depth_lines(name, range(a, b), [9 if p % 7 else 10 for p in range(a, b)])
                     for a, b in ((5, 15), (95, 105), (9990, 10010)))
    rolls += depth_lines(name, range(200, 260), [7, 8, 9, 10, 11, 12] * 10)
    lines = depth_lines(b"NODE_3_length_900_cov_4.5", range(1, 901), (rng.integers(20, 40, 900)).tolist())
    out = [("empty", b""),
           ("one_byte", b"x"),
           ("newlines", b"\n" * MAX_TEXT),
           ("one_value", b"a" * MAX_TEXT),
           ("random", rng.integers(0, 256, MAX_TEXT, dtype=np.uint8).tobytes()),
           ("no_newline", (b"the quick brown fox jumps over the lazy dog " * 300)[:12345]),
           ("rolls", rolls),
           ("mid_line", lines[7:-5]),
           ("fibonacci", fibonacci_piece())]
    assert all(len(p) <= MAX_TEXT for _, p in out) and b"\n" not in out[5][1] and not lines[7:-5].endswith(b"\n")
    return out


def depth_text(n_bytes=1 << 20, seed=5, coverage=30, read_len=150):
    """`samtools depth` text of reads of read_len bases at `coverage` x over contigs named as SPAdes names them"""
    rng = np.random.default_rng(seed)
    parts, total, i = [], 0, 0
    while total < n_bytes:
        i += 1
        L = int(rng.integers(800, 6000))
        n_reads = L * coverage // read_len
        starts = rng.integers(-read_len + 1, L, n_reads)
        diff = np.zeros(L + 1, np.int64)
        np.add.at(diff, np.clip(starts, 0, L), 1)
        np.add.at(diff, np.clip(starts + read_len, 0, L), -1)
        depth = np.cumsum(diff[:-1])
        pos = np.flatnonzero(depth > 0)
        name = b"NODE_%d_length_%d_cov_%.2f" % (i, L, float(depth.mean()))
        parts.append(depth_lines(name, (pos + 1).tolist(), depth[pos].tolist()))
        total += len(parts[-1])
    return b"".join(parts)[:n_bytes]


def cut(text):
    return [text[k:k + MAX_TEXT] for k in range(0, len(text), MAX_TEXT)]
