"""The edge pieces of the BGZF writer's tests (tests/test_host_deflate_enc_edges.py on a CPU, tests/test_gpu_bgzf_deflate_edges.py on
the device): member sizes around every step of `chunk = ceil(n / 512)` and below 512, where most threads own no line; every match
length and every distance code at both of its ends, the copies that overlap themselves and the two distances on either side of
the window; texts on either side of the stored decision; the pieces of tests/deflate_pieces.py; seeded random line-structured
texts.  Every piece is named, seeded and at most 0xff00 bytes.  Test infrastructure."""
import functools

import numpy as np

from tests import deflate_pieces as dp

MAX_TEXT = dp.MAX_TEXT
SIZES = list(range(1, 71)) + [511, 512, 513, 1023, 1024, 1025, 1535, 1536, 1537, 0xfeff, 0xff00]
PAIR_LENGTHS = list(range(3, 262)) + [516, 517, 774]
# the first and the last distance of every distance code (RFC 1951 3.2.5), and the first one past the window
DISTANCES = [1, 2, 3, 4]
for _e in range(1, 14):
    for _half in (0, 1):
        _base = (2 + _half) * (1 << _e) + 1
        DISTANCES += [_base, _base + (1 << _e) - 1]
assert len(DISTANCES) == 56 and DISTANCES[4:8] == [5, 6, 7, 8] and DISTANCES[-4:] == [16385, 24576, 24577, 32768]
TOO_FAR = 32769
DNA = np.frombuffer(b"ACGTacgtNn\t0123456789._", np.uint8)


def _draw(rng, n, alphabet=DNA):
    return alphabet[rng.integers(0, len(alphabet), n)].tobytes()


def _sizes():
    out = []
    for n in SIZES:
        rng = np.random.default_rng(1000 + n)
        body = _draw(rng, n)
        short = bytearray()
        while len(short) < n:                                             # lines of 1 to 3 bytes over two symbols: three or four segments per dword
            short += _draw(rng, int(rng.integers(0, 3)), np.frombuffer(b"ab", np.uint8)) + b"\n"
        out += [(f"size_{n}_no_lf", body), (f"size_{n}_all_lf", b"\n" * n), (f"size_{n}_lf_first", b"\n" + body[1:]),
                (f"size_{n}_lf_last", body[:-1] + b"\n"), (f"size_{n}_short_lines", bytes(short[:n]))]
    return out


def _identical_lines():
    """a line of k bytes (its LF counted) twice: one match of k up to 258, 258 and a rest beyond; and the same line until the piece
    has 1 KiB, which a dynamic block codes shorter than a stored one whatever k is"""
    out = []
    for k in PAIR_LENGTHS:
        line = _draw(np.random.default_rng(2000 + k), k - 1) + b"\n"
        out += [(f"pair_{k}", line * 2), (f"lines_{k}", line * max(3, -(-1024 // k)))]
    return out


def distance_piece(d, seed):
    """a first line of d bytes (its LF counted) and a second one that repeats it with period d for as long as the member allows, at
    least 700 bytes where it does: every copy has distance d, and for d < 258 it overlaps what it writes"""
    if d <= 8:                                                            # the second line is a run of one byte
        first, unit = b"a" * (d - 1) + b"\n", b"a" * d
    else:
        first = _draw(np.random.default_rng(seed), d - 1) + b"\n"
        unit = first[:-1] + b"#"
    room = MAX_TEXT - d
    want = min(max(d + 50, 700), room)
    second = (unit * (want // d + 1))[:want]
    if want < room:
        second += b"\n"
    return first + second


def _distances():
    out = [(f"distance_{d}", distance_piece(d, 3000 + d)) for d in DISTANCES]
    out.append((f"distance_{TOO_FAR}_no_match", distance_piece(TOO_FAR, 3000 + TOO_FAR)))
    return out


def _shapes():
    rng = np.random.default_rng(4000)
    long_line = _draw(rng, 2000) + b"\n"
    line400 = _draw(rng, 399) + b"\n"
    line600 = _draw(rng, 599) + b"\n"
    return [("long_line_between_one_byte_lines", b"\n" * 300 + long_line + b"\n" * 300),
            ("long_line_twice_between_one_byte_lines", b"\n" * 700 + long_line + long_line + b"\n" * 700),
            ("only_lf_is_the_last_byte", _draw(rng, 4999) + b"\n"),
            ("ends_inside_a_match_of_258", line400 + line400[:100]),
            ("ends_inside_the_third_match_of_258", line600 * 2 + line600[:258 + 258 + 40]),
            ("literal_tree_21_levels_deep", deep_piece())]


def deep_piece():
    """21 byte values with frequencies 1, 2, 3, 5, ... 17 711 and no LF: with the end-of-block code as the second 1 every weight is one
    more than the sum of all but the one in front of it, so the optimal tree is a chain 21 levels deep whichever way ties go.  (The
    `fibonacci` piece of deflate_pieces.py has 1, 1, 2, 3, ...: its third 1 lets an optimal tree be 12 levels deep, and the writer's is.)"""
    fib = [1, 2]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    raw = np.concatenate([np.full(f, 65 + i, np.uint8) for i, f in enumerate(fib)])
    np.random.default_rng(4100).shuffle(raw)
    return raw.tobytes()


def _barely():
    """6000 bytes whose first k are drawn from all 255 values but LF and the rest from 128: from clearly coded to clearly stored"""
    every = np.array([v for v in range(256) if v != 10], np.uint8)
    out = []
    for k in range(0, 6001, 500):
        rng = np.random.default_rng(5000 + k)
        out.append((f"barely_{k}", _draw(rng, k, every) + _draw(rng, 6000 - k, every[:128])))
    return out


def random_text(seed):
    """line-structured text of at most 4 KiB: an alphabet of 1 to 255 symbols, lines of 0 to 300 bytes, a line repeated with 0 to 3
    mutations (a byte changed, dropped or put in) or drawn afresh"""
    rng = np.random.default_rng(seed)
    every = np.array([v for v in range(256) if v != 10], np.uint8)
    alphabet = rng.permutation(every)[:int(rng.integers(1, 256))]
    size = int(rng.integers(1, 4097))
    line, out = bytearray(_draw(rng, int(rng.integers(0, 301)), alphabet)), bytearray()
    while len(out) < size:
        out += line + b"\n"
        if rng.random() < 0.25:
            line = bytearray(_draw(rng, int(rng.integers(0, 301)), alphabet))
            continue
        for _ in range(int(rng.integers(0, 4))):
            kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(line) + 1))
            if kind == 0 and at < len(line):
                line[at] = int(alphabet[rng.integers(0, len(alphabet))])
            elif kind == 1 and at < len(line):
                del line[at]
            elif kind == 2 and len(line) < 300:
                line.insert(at, int(alphabet[rng.integers(0, len(alphabet))]))
    return bytes(out[:size])


@functools.lru_cache(maxsize=None)
def cases():
    """((name, bytes), ...)"""
    out = _sizes() + _identical_lines() + _distances() + _shapes() + _barely()
    out += [("piece_" + name, piece) for name, piece in dp.pieces()]
    out += [(f"random_{seed}", random_text(6000 + seed)) for seed in range(100)]
    names = [n for n, _ in out]
    assert len(set(names)) == len(names) and all(len(p) <= MAX_TEXT for _, p in out)
    return tuple(out)
