"""A DEFLATE reader for tests, written from RFC 1951 alone: it shares no line with the inflaters of this tree (csrc/deflate.hpp,
csrc/gzip.hip, host/inflate_fast.hpp) nor with the writer of tests/deflate_streams.py, whose tables it restates from the RFC's
section 3.2.5.  Where zlib tells what a stream MEANS, this tells how it was WRITTEN: per block BFINAL and BTYPE, for a dynamic
block HLIT / HDIST / HCLEN, the three sets of code lengths and the code-length symbols that carried them, and the tokens with the
symbols that coded them.  Everything the RFC forbids raises DeflateError.  Stdlib only, no device.  Test infrastructure."""
from typing import List, NamedTuple, Optional, Tuple


class DeflateError(ValueError):
    pass


# RFC 1951 3.2.5: base and number of extra bits of length symbols 257 .. 285 and of distance symbols 0 .. 29
_LEN = [(3 + i, 0) for i in range(8)]
for _e in range(1, 6):
    for _k in range(4):
        _LEN.append((_LEN[-1][0] + (1 << _LEN[-1][1]), _e))
_LEN.append((258, 0))
_DIST = [(1, 0), (2, 0), (3, 0), (4, 0)]
for _e in range(1, 14):
    for _k in range(2):
        _DIST.append((_DIST[-1][0] + (1 << _DIST[-1][1]), _e))
assert len(_LEN) == 29 and _LEN[27] == (227, 5) and len(_DIST) == 30 and _DIST[29] == (24577, 13)
# 3.2.7: the order in which the lengths of the code-length code are sent
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# 3.2.6: the fixed codes
_FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
_FIXED_DIST = [5] * 32


class Block(NamedTuple):
    final: int
    btype: int
    start_bit: int                       # of BFINAL
    end_bit: int                         # behind the end-of-block code (stored: behind the last byte)
    tokens: list                         # ("lit", byte) / ("match", length, distance); a stored block's bytes as literals
    symbols: list                        # per token: (literal/length symbol, distance symbol or None); stored: empty
    hlit: Optional[int] = None           # dynamic blocks: the counts as they apply (257 .. 286, 1 .. 30, 4 .. 19)
    hdist: Optional[int] = None
    hclen: Optional[int] = None
    cl_lens: Optional[list] = None       # the 19 lengths of the code-length code, by symbol
    cl_syms: Optional[list] = None       # the code-length symbols sent, in order: (symbol, value of its extra bits)
    lit_lens: Optional[list] = None      # hlit entries
    dist_lens: Optional[list] = None     # hdist entries
    header_bits: int = 0                 # from BFINAL to the first token


class Stream(NamedTuple):
    blocks: List[Block]
    bits: int                            # consumed, from the first bit of the first block

    @property
    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


def kraft(lengths, max_bits=15) -> Tuple[int, int]:
    """(sum of 2^(max_bits - l) over the used codes, 2^max_bits): equal when the code is complete"""
    return sum(1 << (max_bits - ln) for ln in lengths if ln), 1 << max_bits


def _table(lengths, what, may_be_lone):
    """decode table of the canonical code of 3.2.2, indexed by the next max-length bits as they lie in the stream (first bit lowest):
    (symbol, length) or None.  -> (table, max length); (None, 0) for no code at all."""
    maxl = max(lengths, default=0)
    if maxl == 0:
        return None, 0
    if maxl > 15:
        raise DeflateError(f"{what}: a code of {maxl} bits")
    have, full = kraft(lengths, maxl)
    if have > full:
        raise DeflateError(f"{what}: over-subscribed code lengths")
    if have < full and not (may_be_lone and maxl == 1):
        raise DeflateError(f"{what}: incomplete code lengths")
    count = [0] * (maxl + 1)
    for ln in lengths:
        count[ln] += 1
    count[0] = 0
    nxt, code = [0] * (maxl + 1), 0
    for bits in range(1, maxl + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    table = [None] * (1 << maxl)
    for sym, ln in enumerate(lengths):
        if not ln:
            continue
        c = nxt[ln]
        nxt[ln] += 1
        rev = int(format(c, "0%db" % ln)[::-1], 2)
        n = 1 << (maxl - ln)
        table[rev::1 << ln] = [(sym, ln)] * n
    return table, maxl


class _Bits:
    def __init__(self, data):
        self.data, self.pos, self.acc, self.n, self.used = bytes(data), 0, 0, 0, 0

    def fill(self, k):
        while self.n < k and self.pos < len(self.data):
            chunk = self.data[self.pos:self.pos + 8]
            self.acc |= int.from_bytes(chunk, "little") << self.n
            self.n += 8 * len(chunk)
            self.pos += len(chunk)

    def take(self, k):
        if self.n < k:
            self.fill(k)
            if self.n < k:
                raise DeflateError("the stream ends inside a block")
        v = self.acc & ((1 << k) - 1)
        self.acc >>= k
        self.n -= k
        self.used += k
        return v

    def symbol(self, table, maxl, what):
        if table is None:
            raise DeflateError(f"{what}: a symbol of a code that has no lengths")
        if self.n < maxl:
            self.fill(maxl)
        e = table[self.acc & ((1 << maxl) - 1)]
        if e is None:
            raise DeflateError(f"{what}: bits that are no code")
        if e[1] > self.n:
            raise DeflateError("the stream ends inside a block")
        self.acc >>= e[1]
        self.n -= e[1]
        self.used += e[1]
        return e[0]


def _dynamic_header(b):
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    if hlit > 286:
        raise DeflateError(f"HLIT says {hlit} literal/length codes")
    if hdist > 30:
        raise DeflateError(f"HDIST says {hdist} distance codes")
    cl_lens = [0] * 19
    for i in range(hclen):
        cl_lens[_CL_ORDER[i]] = b.take(3)
    table, maxl = _table(cl_lens, "code-length code", may_be_lone=False)
    if table is None:
        raise DeflateError("code-length code: no lengths")
    lens, syms = [], []
    while len(lens) < hlit + hdist:
        s = b.symbol(table, maxl, "code-length code")
        if s < 16:
            syms.append((s, 0))
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise DeflateError("repeat of a previous length in front of every length")
            x = b.take(2)
            rep, val = 3 + x, lens[-1]
        elif s == 17:
            x = b.take(3)
            rep, val = 3 + x, 0
        else:
            x = b.take(7)
            rep, val = 11 + x, 0
        syms.append((s, x))
        if len(lens) + rep > hlit + hdist:
            raise DeflateError("a repeat runs past HLIT + HDIST lengths")
        lens += [val] * rep
    lit_lens, dist_lens = lens[:hlit], lens[hlit:]
    if lit_lens[256] == 0:
        raise DeflateError("no end-of-block code")
    return hlit, hdist, hclen, cl_lens, syms, lit_lens, dist_lens


def read(data, before: int = 0, max_out: Optional[int] = None) -> Stream:
    """Every block of the raw DEFLATE stream at the start of `data`, up to and with the block whose BFINAL is set.  before: bytes of
    output in front of the stream that a match may reach; max_out: refuse more output than this."""
    b = _Bits(data)
    blocks, out_len = [], before
    while True:
        start = b.used
        final, btype = b.take(1), b.take(2)
        tokens, symbols = [], []
        if btype == 3:
            raise DeflateError("BTYPE 11")
        if btype == 0:
            b.take((-b.used) % 8)
            ln, nln = b.take(16), b.take(16)
            if ln ^ nln != 0xFFFF:
                raise DeflateError("stored block: NLEN is not the complement of LEN")
            hdr = b.used - start
            assert b.n % 8 == 0
            at = b.pos - b.n // 8
            if at + ln > len(b.data):
                raise DeflateError("the stream ends inside a stored block")
            tokens = [("lit", v) for v in b.data[at:at + ln]]
            b.pos, b.acc, b.n = at + ln, 0, 0
            b.used += 8 * ln
            out_len += ln
            blocks.append(Block(final, 0, start, b.used, tokens, symbols, header_bits=hdr))
        else:
            if btype == 1:
                head = (None,) * 5
                lit_lens, dist_lens = _FIXED_LIT, _FIXED_DIST
            else:
                *head, lit_lens, dist_lens = _dynamic_header(b)
            lit_t, lit_max = _table(lit_lens, "literal/length code", may_be_lone=True)
            dist_t, dist_max = _table(dist_lens, "distance code", may_be_lone=True)
            hdr = b.used - start
            while True:
                s = b.symbol(lit_t, lit_max, "literal/length code")
                if s < 256:
                    tokens.append(("lit", s))
                    symbols.append((s, None))
                    out_len += 1
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise DeflateError(f"length symbol {s}")
                base, extra = _LEN[s - 257]
                length = base + b.take(extra)
                d = b.symbol(dist_t, dist_max, "distance code")
                if d > 29:
                    raise DeflateError(f"distance symbol {d}")
                base, extra = _DIST[d]
                dist = base + b.take(extra)
                if dist > out_len:
                    raise DeflateError(f"distance {dist} behind {out_len} bytes of output")
                tokens.append(("match", length, dist))
                symbols.append((s, d))
                out_len += length
            if btype == 1:
                blocks.append(Block(final, 1, start, b.used, tokens, symbols, header_bits=hdr))
            else:
                blocks.append(Block(final, 2, start, b.used, tokens, symbols, head[0], head[1], head[2], head[3], head[4],
                                    list(lit_lens), list(dist_lens), hdr))
        if max_out is not None and out_len - before > max_out:
            raise DeflateError(f"more than {max_out} bytes of output")
        if final:
            return Stream(blocks, b.used)


def stream_tokens(tokens):
    """the tokens as tests/deflate_streams.py writes them (a literal is an int, a match (length, distance)), for its model()"""
    return [t[1] if t[0] == "lit" else (t[1], t[2]) for t in tokens]
