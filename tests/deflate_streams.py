"""A DEFLATE writer (RFC 1951) and a catalogue of streams written with it by hand -- streams zlib's own encoder never makes, which every
valid stream of the other inflate tests comes from: no distance code at all, a lone distance code of one bit, distance 32 768, length 258
as symbol 284 + 31, 15-bit codes with every extra bit set, a lone end-of-block code, stored blocks behind every bit phase, repeats placed
exactly in the code-length sequence; and the malformed counterparts zlib refuses.  Stdlib + numpy, no device.

A stream is a list of blocks of tokens.  A token is a literal (int), a match `(length, distance[, forced length symbol])`, or -- for
malformed streams only -- `("lit", symbol)` / `("dist", symbol)` (the bare code of a symbol) or `("bits", value, n)`.  `model(tokens)` is
the second statement of what a stream means, independent of zlib; the CPU test holds `model == zlib` on every valid entry.

`python -m tests.deflate_streams` prints the catalogue with zlib's verdict per case."""
import bisect
import functools
import zlib
from typing import NamedTuple, Optional

import numpy as np

from tests.gz_util import gzip_wrap

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
WINDOW = 32768


class BitWriter:
    """bits to bytes, least significant bit first; whole bytes leave the accumulator at once, so it never holds more than a few bits"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, n):
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    @property
    def bit_len(self):
        return len(self.out) * 8 + self.n

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """[(code with its bits reversed, i.e. ready for BitWriter.bits, length) or None] of the canonical code of RFC 1951 3.2.2.  An
    over-subscribed set gets codes cut to their length: such a header is written to be refused, nothing is coded with it."""
    maxl = max(lengths, default=0)
    count = [0] * (maxl + 2)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * (maxl + 2), 0
    for ln in range(1, maxl + 1):
        code = (code + count[ln - 1]) << 1
        nxt[ln] = code
    out = []
    for ln in lengths:
        if ln == 0:
            out.append(None)
            continue
        c = nxt[ln] & ((1 << ln) - 1)
        nxt[ln] += 1
        out.append((int(format(c, "0%db" % ln)[::-1], 2), ln))
    return out


def flat_lengths(n, used):
    """lengths[0 .. n) of a complete code over the symbols `used` (at least two): two neighbouring lengths"""
    used = sorted(set(used))
    k = len(used)
    assert k >= 2
    b = k.bit_length() - 1
    short = (1 << (b + 1)) - k
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = b if i < short else b + 1
    return lens


def rep16(n):
    return (16, n - 3)


def rep17(n):
    return (17, n - 3)


def rep18(n):
    return (18, n - 11)


def write_dynamic_header(w, final, lit_lens, dist_lens, cl_lens=None, hclen=None, cl_syms=None, hlit=None, hdist=None):
    """BFINAL, BTYPE 2 and the code lengths.  cl_syms: the sequence of code-length symbols as (symbol, value of its extra bits) --
    default: every length as itself, no repeats; cl_lens: the 19 lengths of the code-length code -- default: a complete code over the
    symbols of cl_syms; hclen: default the smallest that holds cl_lens; hlit / hdist: what the header says (default: the lists' sizes)."""
    hlit = len(lit_lens) if hlit is None else hlit
    hdist = len(dist_lens) if hdist is None else hdist
    if cl_syms is None:
        cl_syms = [(ln, 0) for ln in list(lit_lens) + list(dist_lens)]
    if cl_lens is None:
        used = {s for s, _ in cl_syms}
        if len(used) == 1:
            used.add(1 if 0 in used else 0)
        cl_lens = flat_lengths(19, used)
    if hclen is None:
        hclen = max(4, 1 + max(i for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    w.bits(final, 1)
    w.bits(2, 2)
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl_lens[CL_ORDER[i]], 3)
    codes = canonical(cl_lens)
    for s, x in cl_syms:
        w.bits(*codes[s])
        if s >= 16:
            w.bits(x, (2, 3, 7)[s - 16])
    return hclen


def length_symbol(length, forced=None):
    """(symbol, value of the extra bits, their number)"""
    if forced is not None:
        c = forced - 257
    elif length == 258:
        c = 28
    else:
        c = bisect.bisect_right(LEN_BASE, length) - 1
    x = length - LEN_BASE[c]
    assert 0 <= x < (1 << LEN_EXTRA[c]) or (x == 0 and LEN_EXTRA[c] == 0), (length, forced)
    return 257 + c, x, LEN_EXTRA[c]


def dist_symbol(d):
    c = bisect.bisect_right(DIST_BASE, d) - 1
    return c, d - DIST_BASE[c], DIST_EXTRA[c]


def write_tokens(w, tokens, lit_codes, dist_codes):
    bits = w.bits
    for t in tokens:
        if isinstance(t, int):
            bits(*lit_codes[t])
        elif t[0] == "lit":
            bits(*lit_codes[t[1]])
        elif t[0] == "dist":
            bits(*dist_codes[t[1]])
        elif t[0] == "bits":
            bits(t[1], t[2])
        else:
            sym, x, nx = length_symbol(t[0], t[2] if len(t) > 2 else None)
            bits(*lit_codes[sym])
            bits(x, nx)
            ds, dx, ndx = dist_symbol(t[1])
            bits(*dist_codes[ds])
            bits(dx, ndx)


def model(tokens, before=b""):
    """the text of a token list; `before`: what lies in front of it (a match may reach into it)"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], str):
            continue
        else:
            length, d = t[0], t[1]
            assert 1 <= d <= len(out), "a match reaches before everything"
            if d >= length:
                s = len(out) - d
                out += out[s:s + length]
            else:
                out += (bytes(out[-d:]) * (length // d + 1))[:length]
    return bytes(out[len(before):])


class Stream:
    """blocks appended one after the other; keeps the tokens of all of them (stored bytes as literals) and every block's first bit"""

    def __init__(self):
        self.w = BitWriter()
        self.tokens = []
        self.starts = []                          # (bit, kind) of every block; kind: 0 stored, 1 fixed, 2 dynamic

    def stored(self, data, final=False, nlen=None):
        self.starts.append((self.w.bit_len, 0))
        self.w.bits(int(final), 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.w.out += data
        self.tokens.extend(data)

    def fixed(self, tokens, final=False, eob=True):
        self.starts.append((self.w.bit_len, 1))
        self.w.bits(int(final), 1)
        self.w.bits(1, 2)
        lit = canonical(FIXED_LIT)
        write_tokens(self.w, tokens, lit, canonical(FIXED_DIST))
        if eob:
            self.w.bits(*lit[256])
        self.tokens.extend(tokens)

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, eob=True, **hdr):
        self.starts.append((self.w.bit_len, 2))
        hclen = write_dynamic_header(self.w, int(final), lit_lens, dist_lens, **hdr)
        lit = canonical(lit_lens)
        write_tokens(self.w, tokens, lit, canonical(dist_lens))
        if eob and len(lit) > 256 and lit[256]:
            self.w.bits(*lit[256])
        self.tokens.extend(tokens)
        return hclen

    def raw(self, pad=0):
        return self.w.bytes() + bytes(pad)

    def text(self, before=b""):
        return model(self.tokens, before)


class Case(NamedTuple):
    name: str
    raw: bytes                    # raw DEFLATE
    text: Optional[bytes]         # what it means; None: zlib refuses it
    out_len: int                  # the size a caller states for it (valid: len(text))
    tail: int = 0                 # bytes of `raw` behind the end of the stream
    why: str = ""                 # invalid: zlib's message ("": the stream is sound and gives one byte more than out_len)


def zlib_says(raw, out_len):
    """(ok, bytes): what zlib makes of a raw stream that should give out_len bytes and end inside `raw`"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw, out_len + 1)
    except zlib.error:
        return False, b""
    return bool(d.eof and len(out) == out_len), out


def zlib_file_says(blob):
    """(text or None, "accepts" or zlib's message) of a whole gzip file: every member, nothing but members"""
    out, rest = [], blob
    try:
        while rest:
            d = zlib.decompressobj(31)
            out.append(d.decompress(rest))
            if not d.eof:
                return None, "truncated"
            rest = d.unused_data
    except zlib.error as e:
        return None, str(e)
    return b"".join(out), "accepts"


def _lits(text):
    return list(text)


FULL_LIT = flat_lengths(286, range(286))
FULL_DIST = flat_lengths(30, range(30))
# a chain of lengths 1, 2, ..., 14, 15, 15: 13 literals, the end-of-block code on 14 bits, length symbols 284 / 285 and distance symbols
# 28 / 29 on the two 15-bit codes
CHAIN_LITERALS = b"ETAOINSHRDLUC"
CHAIN_LIT = [0] * 286
for _i, _c in enumerate(CHAIN_LITERALS):
    CHAIN_LIT[_c] = _i + 1
CHAIN_LIT[256], CHAIN_LIT[284], CHAIN_LIT[285] = 14, 15, 15
CHAIN_DIST = list(range(1, 15)) + [0] * 14 + [15, 15]


def valid_cases():
    rng = np.random.default_rng(1951)
    out = []

    def add(name, s, tail=b""):
        text = s.text()
        out.append(Case(name, s.raw() + tail, text, len(text), len(tail)))

    # ---- code sets zlib's encoder never writes ----
    s = Stream()
    msg = b"no distance code at all: only literals can follow"
    s.dynamic(_lits(msg), flat_lengths(257, set(msg) | {256}), [0], final=True)
    add("no_distance_codes", s)

    s = Stream()
    s.dynamic([97, (258, 1), 98, (5, 1), 97, (3, 1)], flat_lengths(286, {97, 98, 256, 257, 259, 285}), [1], final=True)
    add("lone_distance_code_symbol_0", s)

    s = Stream()
    noise = rng.integers(0, 256, size=WINDOW, dtype=np.uint8).tolist()
    s.dynamic(noise + [(258, 32768), (3, 24577)], flat_lengths(286, set(range(257)) | {257, 285}), [0] * 29 + [1], final=True)
    add("lone_distance_code_symbol_29", s)

    s = Stream()
    s.dynamic([], [0] * 256 + [1], [0], cl_syms=[rep18(138), rep18(118), (1, 0), (0, 0)])
    s.fixed(_lits(b"behind a block whose only code is a 1-bit end-of-block"), final=True)
    add("lone_end_of_block_then_fixed", s)

    s = Stream()
    s.fixed([120, (258, 1, 284), 121, (258, 2, 284)], final=True)
    add("length_258_as_284_plus_31", s)

    s = Stream()
    toks = [CHAIN_LITERALS[min(12, int(g) - 1)] for g in rng.geometric(0.5, size=WINDOW)]
    toks += [(258, 32768, 284), (258, 24576), (227, 1, 284), (258, 32768, 284), 67, (258, 24576)]
    hclen = s.dynamic(toks, CHAIN_LIT, CHAIN_DIST, final=True)
    assert hclen == 19
    add("fifteen_bit_codes_all_extra_bits_set", s)

    s = Stream()
    hclen = s.dynamic(_lits(b"ETAOIN SHRDLU".replace(b" ", b"")), CHAIN_LIT, CHAIN_DIST, final=True)
    assert hclen == 19
    add("hclen_19", s)

    s = Stream()                                  # symbols 16, 17, 18, 0 and 8: no valid block has a shorter code-length list (see invalid_cases)
    hclen = s.dynamic(rng.integers(1, 256, size=300).tolist(), [0] + [8] * 256, [0], final=True)
    assert hclen == 5
    add("hclen_5_the_smallest_of_a_valid_block", s)

    # ---- stored blocks from every bit phase: 10 bits per empty fixed block, 19 for one that holds a 9-bit literal ----
    for odd in (0, 1):
        for k in range(8):
            s = Stream()
            if odd:
                s.fixed([0xF0])
            for _ in range(k):
                s.fixed([])
            phase = s.w.bit_len % 8
            s.stored(b"stored bytes, phase %d" % phase)
            s.fixed(_lits(b"abc") + [(6, 3), (4, 20), 100], final=True)
            add("stored_from_bit_phase_%d_behind_%d_fixed_blocks" % (phase, k + odd), s)
    assert {c.name[22] for c in out if c.name.startswith("stored_from_bit_phase_")} == set("01234567")

    # ---- copies: every distance below, at and above a wavefront's width against lengths below, at and above it ----
    s = Stream()
    toks = [(7 * i + 1) & 255 for i in range(69)]
    for d in range(1, 70):
        for ln in (3, 63, 64, 65, 130, 258):
            toks.append((ln, d))
    s.fixed(toks, final=True)
    add("distances_1_to_69_by_lengths_3_to_258", s)

    s = Stream()
    s.fixed([97, 98, 99, (3, 3), 100, (7, 7), (14, 14), 101], final=True)
    add("distance_equal_to_the_output_so_far", s)

    s = Stream()
    s.fixed([97, 98, (258, 2)], final=True)
    add("match_ends_at_out_len", s)

    s = Stream()
    s.fixed([122] + [(258, 1)] * 254 + [(3, 1)], final=True)
    assert len(s.text()) == 65536
    add("member_of_65536_bytes", s)

    s = Stream()
    s.stored(b"")
    s.stored(bytes(rng.integers(0, 256, size=65535, dtype=np.uint8)))
    s.fixed([33], final=True)
    assert len(s.text()) == 65536
    add("stored_blocks_of_0_and_65535_bytes", s)

    s = Stream()
    s.stored(b"", final=True)
    add("one_empty_stored_block", s)

    # ---- headers ----
    s = Stream()
    toks = list(range(256)) + rng.integers(0, 256, size=WINDOW, dtype=np.uint8).tolist()
    for i in range(30):
        c = i % 29
        toks.append((LEN_BASE[c] + (1 << LEN_EXTRA[c]) - 1, DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1, 257 + c))
        toks.append(int(rng.integers(0, 256)))
    s.dynamic(toks, FULL_LIT, FULL_DIST, final=True)
    add("hlit_286_hdist_30_every_symbol_used", s)

    s = Stream()
    lit = [0] * 286
    for c in list(range(65, 90)) + [256] + list(range(280, 286)):
        lit[c] = 5
    dist = [5] * 28 + [4, 4]
    syms = [rep18(65), (5, 0)] + [rep16(6)] * 4 + [rep18(138), rep18(28), (5, 0), rep18(23), (5, 0),
            rep16(6),                            # symbols 281 .. 285 and distance symbol 0
            rep16(6), rep16(6), rep16(6), rep16(6), rep16(3), (4, 0), (4, 0)]
    toks = list(range(65, 90)) + [(115, 25), (131, 100), (258, 7), (163, 200), 70, (195, 1), (227, 300), (146, 512), 71]
    s.dynamic(toks, lit, dist, final=True, cl_syms=syms)
    add("repeat_16_crosses_from_lengths_to_distances", s)

    s = Stream()
    lit = [1] + [0] * 255 + [2] + [0] * 6 + [3] + [0] * 20 + [3]          # literal 0, end-of-block, 263 (length 9), 284: HLIT = 285
    assert len(lit) == 285
    syms = [(1, 0), rep18(138), rep18(117), (2, 0), rep17(6), (3, 0), rep18(20), (3, 0), (1, 0)]
    s.dynamic([0, (258, 1, 284), 0, 0, (9, 1)], lit, [1], final=True, cl_syms=syms)
    add("repeat_18_runs_of_138_and_117", s)

    # ---- the end of the stream ----
    s = Stream()
    s.fixed([0x90, 0xA1, 0xB2, 0xC3, 0xD4, 0xE5], final=True)              # 3 + 6 * 9 + 7 bits
    assert s.w.bit_len % 8 == 0 and s.w.bit_len == 64
    add("last_bit_is_the_last_bit_of_the_last_byte", s)
    add("the_same_with_five_bytes_behind_it", s, tail=b"\xff\x00\xa5\x5a\xff")
    return out


def invalid_cases():
    out = []

    def add(name, s, why, out_len=16):
        out.append(Case(name, s.raw(pad=6 if why else 0), None, out_len, 0, why))     # (zeros behind a malformed stream: it is refused, not cut short)

    ab = flat_lengths(257, {97, 98, 256})
    s = Stream()
    s.dynamic([], ab, [0], final=True, cl_lens=[1] + [0] * 18, cl_syms=[(0, 0)] * 258)
    add("lone_code_length_code", s, "invalid code lengths set")

    s = Stream()
    s.dynamic([97, ("lit", 257), ("bits", 0, 8)], flat_lengths(258, {97, 256, 257}), [0], final=True)
    add("distance_used_without_distance_codes", s, "invalid distance code")

    s = Stream()
    s.dynamic([97, ("lit", 257), ("bits", 1, 1)], flat_lengths(258, {97, 256, 257}), [1], final=True)
    add("unused_bit_pattern_of_a_lone_distance_code", s, "invalid distance code")

    s = Stream()
    lit = [0] * 257
    lit[97] = lit[256] = 2
    s.dynamic([97], lit, [0], final=True)
    add("incomplete_literal_set_of_two_2_bit_codes", s, "invalid literal/lengths set")

    s = Stream()
    s.fixed([97, ("lit", 286)], final=True)
    add("fixed_code_symbol_286", s, "invalid literal/length code")

    s = Stream()
    s.fixed([97, 98, ("lit", 257), ("dist", 30)], final=True)
    add("fixed_distance_30", s, "invalid distance code")

    s = Stream()
    s.w.bits(1, 1)
    s.w.bits(3, 2)
    add("btype_3", s, "invalid block type")

    s = Stream()
    s.stored(b"sixteen bytes ..", final=True, nlen=(16 ^ 0xFFFF) ^ 0x0100)
    add("len_nlen_mismatch", s, "invalid stored block lengths")

    s = Stream()
    lit = [0] * 257
    lit[97] = lit[98] = lit[256] = 1
    s.dynamic([], lit, [0], final=True)
    add("oversubscribed_literal_set", s, "invalid literal/lengths set")

    s = Stream()
    s.dynamic([], ab, [1, 1, 1], final=True)
    add("oversubscribed_distance_set", s, "invalid distances set")

    s = Stream()
    s.dynamic([], ab, [0], final=True, cl_lens=[1, 1, 1] + [0] * 16)
    add("oversubscribed_code_length_set", s, "invalid code lengths set")

    s = Stream()
    s.dynamic([97, 98], flat_lengths(257, {97, 98}), [0], final=True)
    add("no_end_of_block_code", s, "missing end-of-block")

    s = Stream()
    s.dynamic([], ab, [0], final=True, cl_lens=flat_lengths(19, {0, 1, 16}), cl_syms=[rep16(3)] + [(1, 0)] * 255)
    add("repeat_16_as_the_first_symbol", s, "invalid bit length repeat")

    s = Stream()
    s.dynamic([], [1] + [0] * 255 + [1], [1], final=True, cl_syms=[(1, 0), rep18(138), rep18(117), (1, 0), rep17(3)])
    add("repeat_runs_past_hlit_plus_hdist", s, "invalid bit length repeat")

    for hlit in (287, 288):
        s = Stream()
        s.dynamic([], FULL_LIT, [0], final=True, hlit=hlit)
        add("hlit_%d" % hlit, s, "too many length or distance symbols")
    for hdist in (31, 32):
        s = Stream()
        s.dynamic([], ab, FULL_DIST, final=True, hdist=hdist)
        add("hdist_%d" % hdist, s, "too many length or distance symbols")

    # HCLEN = 4 names lengths for the symbols 16, 17, 18 and 0 alone: every code length is then 0, the end-of-block code among them, so no
    # valid block has it (the smallest HCLEN of a valid block is 5: valid_cases)
    s = Stream()
    s.dynamic([], [0] * 257, [0], final=True, cl_lens=flat_lengths(19, {0, 18}), hclen=4, cl_syms=[rep18(138), rep18(119), (0, 0)])
    add("hclen_4", s, "missing end-of-block")

    s = Stream()
    s.w.bits(1, 1)
    s.w.bits(1, 2)
    lit, dist = canonical(FIXED_LIT), canonical(FIXED_DIST)
    write_tokens(s.w, [97, 98, 99, (3, 4)], lit, dist)
    s.w.bits(*lit[256])
    add("distance_is_the_output_so_far_plus_1", s, "invalid distance too far back", out_len=6)

    s = Stream()
    s.fixed([97, (10, 1)], final=True)
    add("match_one_byte_longer_than_out_len", s, "", out_len=10)
    return out


# ------------------------------------------------------------------------------------------------
# long streams for the gzip path: tokens written directly, no match search
# ------------------------------------------------------------------------------------------------
class Long(NamedTuple):
    name: str
    raw: bytes
    text: bytes
    starts: list                  # (bit, kind) of every block


def _long_stream(kind, seed, n_blocks=90, n_lit=2400):
    rng = np.random.default_rng(seed)
    s = Stream()
    total = 0                                     # text so far
    lit_only = flat_lengths(257, range(257))

    def literals(n):
        return rng.integers(0, 256, size=n, dtype=np.uint8).tolist()

    def full_block(first_far):
        """literals and matches of every distance; first_far: the block's first token is a match of distance 32 768 (the first byte of the
        window before the block) and a later one has distance = its position in the block + 1 (the last byte of that window)"""
        nonlocal total
        toks, at = [], 0                          # at: text of this block so far

        def match(ln, d):
            nonlocal at
            toks.append((ln, d))
            at += ln

        if first_far and total >= WINDOW:
            match(int(rng.choice([3, 64, 258])), WINDOW)
        n = 0
        while n < n_lit:
            k = int(rng.integers(20, 61))
            toks.extend(literals(k))
            n += k
            at += k
            have = total + at
            if first_far and total >= WINDOW and at < 2000 and n >= 600 and not any(isinstance(t, tuple) and t[1] == at + 1 for t in toks[-3:]):
                match(int(rng.integers(3, 259)), at + 1)
                first_far = False
                continue
            pick = int(rng.integers(0, 4))
            d = WINDOW if pick == 0 else int(rng.integers(1, 70)) if pick == 1 else int(rng.integers(1, WINDOW + 1))
            match(int(rng.integers(3, 259)), min(d, have))
        total += at
        return toks

    for b in range(n_blocks):
        if kind == "a":
            s.dynamic(full_block(True), FULL_LIT, FULL_DIST)
        elif kind == "b":
            if b % 3 == 0:                        # no distance code at all
                s.dynamic(literals(n_lit), lit_only, [0])
                total += n_lit
            elif b % 3 == 1:                      # a lone distance code: symbol 0 (distance 1), or symbol 29 (24 577 .. 32 768)
                toks, far = [], (b % 2 == 0 and total >= WINDOW)
                for _ in range(40):
                    toks.extend(literals(60))
                    ln = int(rng.integers(3, 259))
                    toks.append((ln, int(rng.integers(24577, WINDOW + 1)) if far else 1))
                    total += 60 + ln
                s.dynamic(toks, FULL_LIT, [0] * 29 + [1] if far else [1])
            else:
                s.dynamic(full_block(False), FULL_LIT, FULL_DIST)
        else:                                     # fixed, stored and lone end-of-block blocks between the dynamic ones
            s.dynamic(full_block(b % 2 == 0), FULL_LIT, FULL_DIST)
            what = b % 4
            if what == 0:
                toks = literals(b % 7) + [(5, 1)]
                s.fixed(toks)
                total += len(toks) - 1 + 5
            elif what == 1:
                data = bytes(literals(b % 50))
                s.stored(data)
                total += len(data)
                s.fixed(literals(b % 5))
                total += b % 5
            elif what == 2:
                s.dynamic([], [0] * 256 + [1], [0], cl_syms=[rep18(138), rep18(118), (1, 0), (0, 0)])
            else:
                s.fixed([])
                s.dynamic([], [0] * 256 + [1], [0], cl_syms=[rep18(138), rep18(118), (1, 0), (0, 0)])
    s.fixed([10], final=True)
    text = s.text()
    assert len(text) == total + 1
    return Long("long_" + kind, s.raw(), text, s.starts)


@functools.lru_cache(maxsize=None)
def long_streams():
    """(a) matches of distance 32 768 and of the first and last byte of the window before every block; (b) blocks without distance codes,
    with a lone one and with all of them in turns; (c) fixed, stored and lone end-of-block blocks between the dynamic ones"""
    return tuple(_long_stream(k, 100 + i) for i, k in enumerate("abc"))


@functools.lru_cache(maxsize=None)
def catalogue():
    return tuple(valid_cases() + invalid_cases())


# ------------------------------------------------------------------------------------------------
# gzip files whose matches reach before the start of their member
# ------------------------------------------------------------------------------------------------
REACH_FIRST_BLOCK = 17000          # literals of the first block: more than 16 KiB of compressed data, fewer than 32 768 bytes of text
REACH_DISTANCE = 30000


def _reach_before_member(seed, before):
    """(raw, text as a decoder without the check would give it): a first block of 17 000 literals at 8 bits each, then a non-final dynamic
    block whose first token is a match of distance 30 000 -- 13 000 bytes before the member's start, where `before` lies"""
    rng = np.random.default_rng(seed)
    s = Stream()
    s.dynamic(rng.integers(0, 255, size=REACH_FIRST_BLOCK, dtype=np.uint8).tolist(), flat_lengths(257, range(257)), [0])
    assert s.w.bit_len > 8 * (16 << 10) + 64
    toks = [(100, REACH_DISTANCE)]
    for _ in range(30):
        toks += rng.integers(0, 256, size=40, dtype=np.uint8).tolist() + [(int(rng.integers(3, 259)), int(rng.integers(1, 2000)))]
    s.dynamic(toks, FULL_LIT, FULL_DIST)
    s.dynamic(rng.integers(0, 256, size=1500, dtype=np.uint8).tolist(), FULL_LIT, FULL_DIST)
    s.fixed([10], final=True)
    return s.raw(), s.text(before=before), s.starts


@functools.lru_cache(maxsize=None)
def reach_before_files():
    """{name: (file, the bit of the file at which the offending block starts, the byte at which its member starts)}.  Every trailer carries the CRC-32 and ISIZE of the text a
    decoder gives that resolves the reference from what lies before the member: zeros, or the previous member's text."""
    out = {}
    raw, text, starts = _reach_before_member(7, bytes(WINDOW))
    out["one_member"] = (gzip_wrap(raw, text), 80 + starts[1][0], 0)
    first = next(c for c in catalogue() if c.name == "lone_distance_code_symbol_29")
    m1 = gzip_wrap(first.raw, first.text)
    raw, text, starts = _reach_before_member(8, bytes(WINDOW) + first.text)
    out["second_of_two_members"] = (m1 + gzip_wrap(raw, text), 8 * (len(m1) + 10) + starts[1][0], len(m1))
    return out


def main():
    for c in catalogue():
        ok, got = zlib_says(c.raw, c.out_len)
        verdict = "accepts" if ok else "refuses"
        agree = "" if ok == (c.text is not None) and (not ok or got == c.text) else "   <-- NOT what the catalogue says"
        print("%-50s %6d -> %6d bytes  zlib %s%s" % (c.name, len(c.raw), c.out_len, verdict, agree))
    for g in long_streams():
        ok, got = zlib_says(g.raw, len(g.text))
        print("%-50s %6d -> %6d bytes  zlib %s, %d blocks" % (g.name, len(g.raw), len(g.text), "accepts" if ok and got == g.text else "DISAGREES", len(g.starts)))
    for name, (blob, bit, _) in reach_before_files().items():
        msg = zlib_file_says(blob)[1]
        print("%-50s %6d bytes, offending block at bit %d  zlib: %s" % ("reach_before_" + name, len(blob), bit, msg))


if __name__ == "__main__":
    main()
