"""An exact model of the BGZF writer (palace_bgzf_deflate; csrc/deflate_enc.hpp on a CPU), restated from its rules as the head of
deflate_enc.hpp, DESIGN.md and include/palace_hip.h give them -- not from its code:

* tokens: the match candidate of a byte is the byte one previous-line-length back (a line ends with its LF; the last line of a
  member may lack one); the walk over a line is greedy; a match has 3 .. 258 bytes and ends with its line at the latest; the first
  line of a member, and a line behind one longer than 32 768 bytes, has literals only.  The rules allow ONE token sequence.
* codes: Huffman codes of the member's own histograms, so the coded size is the optimum wherever the optimal tree fits the limit of
  15 / 15 / 7 bits.  The optimum and the least depth an optimal tree can have come from a heap, not from the writer's in-place method.
* a piece is stored when the dynamic block would not be shorter than 5 + n bytes.

Plain Python: a 64 KiB piece takes a tenth of a second.  Test infrastructure."""
import heapq

MAX_TEXT = 0xff00
WINDOW = 32768
MIN_MATCH, MAX_MATCH = 3, 258
LF = 10


def tokens_of(text):
    """[("lit", byte) | ("match", length, distance)] of one member's text"""
    text = bytes(text)
    n, out = len(text), []
    start, prev_len = 0, 0                     # of the current line; length of the line in front of it (its LF counted), 0 = none
    while start < n:
        lf = text.find(b"\n", start)
        end = n if lf < 0 else lf + 1          # the line is text[start:end]
        p = start
        if 0 < prev_len <= WINDOW:
            d = prev_len
            while p < end:
                limit = min(end - p, MAX_MATCH)
                r = 0
                while r < limit and text[p + r] == text[p + r - d]:
                    r += 1
                if r >= MIN_MATCH:
                    out.append(("match", r, d))
                    p += r
                else:
                    out.append(("lit", text[p]))
                    p += 1
        else:
            out.extend(("lit", v) for v in text[start:end])
        prev_len, start = end - start, end
    return out


def text_of(tokens):
    """the text a token list stands for (RFC 1951 3.2.3: a copy may overlap what it writes)"""
    out = bytearray()
    for t in tokens:
        if t[0] == "lit":
            out.append(t[1])
        else:
            _, length, d = t
            assert 1 <= d <= len(out)
            for _ in range(length):
                out.append(out[-d])
    return bytes(out)


def length_symbol(length):
    """(symbol 257 .. 285, extra bits, their value) of a match length, RFC 1951 3.2.5"""
    assert MIN_MATCH <= length <= MAX_MATCH
    if length == 258:
        return 285, 0, 0
    sym, base = 257, 3
    for extra in (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4:
        if length < base + (1 << extra):
            return sym, extra, length - base
        sym, base = sym + 1, base + (1 << extra)
    raise AssertionError(length)


def distance_symbol(d):
    """(symbol 0 .. 29, extra bits, their value) of a distance"""
    assert 1 <= d <= WINDOW
    sym, base = 0, 1
    for extra in (0,) * 4 + tuple(e for e in range(1, 14) for _ in (0, 1)):
        if d < base + (1 << extra):
            return sym, extra, d - base
        sym, base = sym + 1, base + (1 << extra)
    raise AssertionError(d)


def histograms(tokens):
    """(literal/length frequencies [286] with the end-of-block code counted once, distance frequencies [30], extra bits in all)"""
    lit, dist, extra = [0] * 286, [0] * 30, 0
    lit[256] = 1
    for t in tokens:
        if t[0] == "lit":
            lit[t[1]] += 1
        else:
            s, e, _ = length_symbol(t[1])
            lit[s] += 1
            extra += e
            s, e, _ = distance_symbol(t[2])
            dist[s] += 1
            extra += e
    return lit, dist, extra


def huffman_cost(freqs):
    """(total bits of an optimal prefix code for the non-zero frequencies, the least depth an optimal tree can have).  One used
    symbol costs one bit a time (DEFLATE has no code of zero bits); none costs nothing.  Ties go to the shallower subtree, which
    gives the optimal tree of the least height."""
    used = [f for f in freqs if f]
    if not used:
        return 0, 0
    if len(used) == 1:
        return used[0], 1
    heap = [(f, 0) for f in used]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        total += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return total, heap[0][1]


def coded_bits(freqs, lengths):
    return sum(f * ln for f, ln in zip(freqs, lengths))


def monotone(freqs, lengths):
    """a symbol that is more frequent never has the longer code (among the used symbols)"""
    span = {}
    for f, ln in zip(freqs, lengths):
        if f:
            lo, hi = span.get(f, (ln, ln))
            span[f] = (min(lo, ln), max(hi, ln))
    by_freq = [span[f] for f in sorted(span)]
    return all(a[0] >= b[1] for a, b in zip(by_freq, by_freq[1:]))
