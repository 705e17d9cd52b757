"""The pieces of the tests of the BGZF writer's hashed matcher (palace_bgzf_deflate_lz; tests/test_host_deflate_lz.py on a CPU,
tests/test_gpu_bgzf_deflate_lz.py on the device): the smallest shapes at which the rule of csrc/deflate_lz.hpp can still go wrong --
pieces shorter than the hash window, around one and two rounds of R = 512 positions, the largest members, overlapping copies, the
window's edge, repeats against the chunk borders, a source inside the copy's own round, two strings of one bucket, noise, and a piece
shaped like a BAM.  Every piece is named, seeded and at most 0xff00 bytes; `PLANTED` says where the planted bytes lie, for the tests
that look at the model's tokens there.  Test infrastructure."""
import functools
import struct

import numpy as np

from tests import deflate_lz_model as lz

MAX_TEXT = 0xff00
R = lz.R
FILL = b"\0"


def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _words(seed, n):
    """low-entropy text without lines: words of a small vocabulary"""
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.integers(97, 101, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(12)]
    out = bytearray()
    while len(out) < n:
        out += vocab[int(rng.integers(0, len(vocab)))]
    return bytes(out[:n])


def planted(n, parts):
    """n bytes of filler with `parts` = [(position, bytes)] written over it"""
    out = bytearray(FILL * n)
    for at, data in parts:
        assert 0 <= at and at + len(data) <= n
        out[at:at + len(data)] = data
    return bytes(out)


def repeat_piece(n, src, dst, block):
    """filler with `block` at src and at dst; the byte behind the copy is not the byte behind the source, so no match runs on past it"""
    return planted(n, [(src, block), (dst, block + b"\xff")])


@functools.lru_cache(maxsize=None)
def colliding_words():
    """two different 4-byte strings of one bucket, neither holding the filler's byte: found by search"""
    seen = {}
    for k in range(1 << 20):
        w = b"%04d" % k if k < 10000 else struct.pack("<I", 0x41414141 + 2654435 * k)
        if 0 in w:
            continue
        h = lz.hash4(w)
        if h in seen and seen[h] != w:
            return seen[h], w
        seen.setdefault(h, w)
    raise AssertionError("no collision found")


def bam_shaped(seed=77, records=400):
    """BAM records as an aligner leaves them: names with a shared prefix, one CIGAR operation, packed bases, qualities in runs"""
    rng = np.random.default_rng(seed)
    out, pos = bytearray(), 1000
    for k in range(records):
        name = b"HWI-ST1234:100:C0ABCACXX:1:1101:%d:%d\0" % (1200 + 3 * (k // 2), 2000 + 7 * (k // 2))
        l_seq = 100
        pos += int(rng.integers(0, 40))
        flag = (99, 147)[k & 1]
        seq = rng.integers(0, 4, (l_seq + 1) // 2 * 2, dtype=np.uint8)
        packed = ((1 << seq[0::2]) << 4 | (1 << seq[1::2])).astype(np.uint8).tobytes()
        qual = bytearray()
        while len(qual) < l_seq:
            qual += bytes([int(rng.choice([2, 30, 37, 40, 41]))]) * int(rng.integers(1, 30))
        body = struct.pack("<iiBBHHHIiii", 0, pos, len(name), 60, 4681, 1, flag, l_seq, 0, pos + 150, 250) + name + struct.pack("<I", l_seq << 4) + packed + bytes(qual[:l_seq])
        body += b"NMC\0" + b"ASC" + bytes([l_seq])
        out += struct.pack("<I", len(body)) + body
    return bytes(out[:MAX_TEXT])


# name -> (position of the copy, its length): where the tests look at the model's tokens
PLANTED = {}


@functools.lru_cache(maxsize=None)
def cases():
    """((name, bytes), ...)"""
    out = [("empty", b"")]
    out += [(f"size_{n}", _words(100 + n, n)) for n in (1, 2, 3, 4, 5, R - 1, R, R + 1, 2 * R + 3, 7 * R + 1, MAX_TEXT - 1, MAX_TEXT)]
    out += [("one_byte_run", b"A" * MAX_TEXT), ("period_2", (b"ab" * MAX_TEXT)[:MAX_TEXT - 3]), ("period_3", (b"xyz" * MAX_TEXT)[:MAX_TEXT - 7])]

    # the window's edge: a block of noise and its copy 32768 and 32769 bytes behind it
    block = _noise(1, 300)
    for d in (32768, 32769):
        out.append((f"distance_{d}", repeat_piece(700 + d + 400, 700, 700 + d, block)))
        PLANTED[f"distance_{d}"] = (700 + d, len(block))

    # repeats of 258, 259 and 600 bytes whose source lies rounds back: chunk = ceil(20000 / 512) = 40 bytes, so every one is cut at
    # the chunk borders (the cap of 258 cannot bind below 512 * 258 bytes of text, and a member has at most 0xff00)
    for k in (258, 259, 600):
        out.append((f"repeat_{k}", repeat_piece(20000, 1000, 9000, _noise(10 + k, k))))
        PLANTED[f"repeat_{k}"] = (9000, k)
    # a repeat of 30 bytes inside one chunk of 40, and the same across a border: [9000, 9040) is a chunk
    out += [("repeat_inside_a_chunk", repeat_piece(20000, 1000, 9005, _noise(20, 30))), ("repeat_across_a_chunk_border", repeat_piece(20000, 1000, 9025, _noise(20, 30)))]
    PLANTED["repeat_inside_a_chunk"], PLANTED["repeat_across_a_chunk_border"] = (9005, 30), (9025, 30)
    # the source in the copy's own round [1024, 1536), and in the round before it
    out += [("source_in_the_same_round", repeat_piece(4000, 1030, 1200, _noise(21, 60))), ("source_in_the_round_before", repeat_piece(4000, 900, 1200, _noise(21, 60)))]
    PLANTED["source_in_the_same_round"], PLANTED["source_in_the_round_before"] = (1200, 60), (1200, 60)

    a, b = colliding_words()
    out.append(("equal_hash_different_bytes", planted(4000, [(100, a), (1200, b)])))
    PLANTED["equal_hash_different_bytes"] = (1200, 4)

    out += [("noise", _noise(30, 5000)), ("bam_shaped", bam_shaped())]
    names = [n for n, _ in out]
    assert len(set(names)) == len(names) and all(len(p) <= MAX_TEXT for _, p in out)
    return tuple(out)


def tokens_at(piece, at, length):
    """the model's tokens that cover bytes [at, at + length) of the piece: [(position, token)]"""
    out, p = [], 0
    for t in lz.tokens_of(piece):
        k = 1 if t[0] == "lit" else t[1]
        if p < at + length and p + k > at:
            out.append((p, t))
        p += k
    return out
