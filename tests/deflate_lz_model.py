"""An exact model of the BGZF writer's second coder (palace_bgzf_deflate_lz; csrc/deflate_lz.hpp over csrc/deflate_enc.hpp), restated
from the rules as the heads of those headers, DESIGN.md 8 and include/palace_hip.h give them -- not from their code:

* hash: h(p) = the top 14 bits of (the little-endian 32-bit word of bytes p .. p + 3) * 2654435761 mod 2^32, for p <= n - 4;
* candidate: the member is taken in rounds of R = 512 positions; cand(p) is the greatest q with h(q) == h(p), q < R * floor(p / R) and
  p - q <= 32768, or none -- never a position of p's own round;
* tokens: thread t owns bytes [t * chunk, (t + 1) * chunk), chunk = ceil(n / R), and parses them greedily from its first byte; the
  match length is the count of equal bytes at the candidate, capped at 258, at the member's end and at the chunk's end; under 3 it is
  a literal; after a match parsing resumes behind it;
* codes: frequencies sorted by (frequency, symbol), in-place Moffat-Katajainen, lengths limited to 15 / 15 / 7 bits by moving codes
  between the length classes until the Kraft sum is exact, canonical codes; a member without a match declares one distance code of
  one bit; a code-length alphabet with one used symbol gets a second one; the header lists the lengths one by one;
* a piece is stored when the dynamic block would not be shorter than 5 + n bytes; an empty piece is the EOF member.

The histograms, the symbols and the bit writer are those of tests/deflate_enc_model.py and tests/deflate_streams.py.  Plain Python.
Test infrastructure."""
import functools
import struct
import zlib

from tests import deflate_enc_model as dm
from tests import deflate_read as dr
from tests import deflate_streams as ds
from tests import tabix_reader as tr

R = 512
HASH_BITS = 14
WINDOW = dm.WINDOW
MIN_MATCH, MAX_MATCH = dm.MIN_MATCH, dm.MAX_MATCH
HEADER = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00"


def hash4(four):
    """bucket of the four bytes `four`"""
    return ((int.from_bytes(four, "little") * 2654435761) & 0xffffffff) >> (32 - HASH_BITS)


def chunk_of(n):
    return -(-n // R)


def distances(text):
    """dist[p] = p - cand(p), or 0 where p has no candidate"""
    n = len(text)
    dist, head = [0] * n, {}
    for start in range(0, n, R):
        ps = range(start, min(start + R, n - 3))
        hs = [hash4(text[p:p + 4]) for p in ps]
        for p, h in zip(ps, hs):                      # the whole round looks ...
            q = head.get(h)
            if q is not None and p - q <= WINDOW:
                dist[p] = p - q
        for p, h in zip(ps, hs):                      # ... before any of it enters (ascending: the greatest stays)
            head[h] = p
    return dist


def tokens_of(text):
    """[("lit", byte) | ("match", length, distance)] of one member's text"""
    text = bytes(text)
    n, out = len(text), []
    if n == 0:
        return out
    dist, chunk = distances(text), chunk_of(n)
    for c0 in range(0, n, chunk):
        c1, p = min(c0 + chunk, n), c0
        while p < c1:
            d, r = dist[p], 0
            if d:
                cap = min(MAX_MATCH, c1 - p)
                while r < cap and text[p + r] == text[p + r - d]:
                    r += 1
            if r >= MIN_MATCH:
                out.append(("match", r, d))
                p += r
            else:
                out.append(("lit", text[p]))
                p += 1
    return out


def code_lengths(freqs, limit):
    """the writer's code lengths of a histogram: Moffat-Katajainen on the used symbols in the order (frequency, symbol), then the limit"""
    order = sorted((f, s) for s, f in enumerate(freqs) if f)
    n, lens = len(order), [0] * len(freqs)
    if n == 0:
        return lens
    num = [0] * (limit + 2)
    if n == 1:
        num[1] = 1
    else:
        a = [f for f, _ in order]
        a[0] += a[1]
        root, leaf = 0, 2
        for nxt in range(1, n - 1):
            if leaf >= n or a[root] < a[leaf]:
                a[nxt] = a[root]
                a[root] = nxt
                root += 1
            else:
                a[nxt] = a[leaf]
                leaf += 1
            if leaf >= n or (root < nxt and a[root] < a[leaf]):
                a[nxt] += a[root]
                a[root] = nxt
                root += 1
            else:
                a[nxt] += a[leaf]
                leaf += 1
        a[n - 2] = 0
        for nxt in range(n - 3, -1, -1):
            a[nxt] = a[a[nxt]] + 1
        avbl, used, depth, root, nxt = 1, 0, 0, n - 2, n - 1
        while avbl > 0:
            while root >= 0 and a[root] == depth:
                used += 1
                root -= 1
            while avbl > used:
                a[nxt] = depth
                nxt -= 1
                avbl -= 1
            avbl, depth, used = 2 * used, depth + 1, 0
        for d in a:
            num[min(d, limit)] += 1
        total = sum(num[i] << (limit - i) for i in range(1, limit + 1))
        while total != 1 << limit:                    # one of the longest leaves, a shorter code takes its sibling
            num[limit] -= 1
            for i in range(limit - 1, 0, -1):
                if num[i]:
                    num[i] -= 1
                    num[i + 1] += 2
                    break
            total -= 1
    j = n
    for i in range(1, limit + 1):                     # the most frequent symbols get the shortest codes
        for _ in range(num[i]):
            j -= 1
            lens[order[j][1]] = i
    return lens


def block_of(tokens):
    """(the dynamic block of the tokens as bytes, its length in bits)"""
    lit, dist, _ = dm.histograms(tokens)
    lit_lens = code_lengths(lit, 15)
    nlit = max(i for i in range(286) if lit_lens[i]) + 1
    dist_lens = code_lengths(dist, 15)
    if not any(dist):
        dist_lens[0] = 1
    ndist = max(i for i in range(30) if dist_lens[i]) + 1
    sent = lit_lens[:nlit] + dist_lens[:ndist]
    cl = [0] * 19
    for ln in sent:
        cl[ln] += 1
    if sum(1 for f in cl if f) == 1:
        cl[1 if cl[0] else 0] = 1
    cl_lens = code_lengths(cl, 7)
    w = ds.BitWriter()
    ds.write_dynamic_header(w, 1, lit_lens[:nlit], dist_lens[:ndist], cl_lens=cl_lens)
    lit_codes = ds.canonical(lit_lens)
    ds.write_tokens(w, dr.stream_tokens(tokens), lit_codes, ds.canonical(dist_lens))
    w.bits(*lit_codes[256])
    return w.bytes(), w.bit_len


@functools.lru_cache(maxsize=None)
def member_of(piece):
    """the member of a piece, byte for byte"""
    piece = bytes(piece)
    n = len(piece)
    if n == 0:
        return tr.EOF_MEMBER
    block, bits = block_of(tokens_of(piece))
    if (bits + 7) // 8 >= 5 + n:
        block = b"\x01" + struct.pack("<HH", n, n ^ 0xffff) + piece
    total = 18 + len(block) + 8
    return HEADER + struct.pack("<H", total - 1) + block + struct.pack("<II", zlib.crc32(piece), n)


def has_match(member):
    """the member's block is a dynamic one with at least one match token"""
    b = dr.read(member[18:len(member) - 8]).blocks[0]
    return b.btype == 2 and any(t[0] == "match" for t in b.tokens)
