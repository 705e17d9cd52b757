"""What a BGZF member of the writer (palace_bgzf_deflate; csrc/deflate_enc.hpp on a CPU) must be, checked with the reader written
from the RFC (tests/deflate_read.py) against the exact model (tests/deflate_enc_model.py): framing, the one token sequence the rules
allow, trimmed counts, complete codes within 15 / 15 / 7 bits, the optimal coded size wherever the optimal tree fits, and the
stored decision.  Shared by tests/test_host_deflate_enc_edges.py and tests/test_gpu_bgzf_deflate_edges.py.  Test infrastructure."""
import functools
import os
import struct
import subprocess
import zlib

from tests import deflate_enc_model as dm
from tests import deflate_read as dr
from tests import tabix_reader as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
TOOL = os.path.join(ROOT, "palace_amd", "bin", "deflate_selftest")
TOOL_ASAN = TOOL + "_asan"
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)        # RFC 1951 3.2.7
# the most a dynamic block's header can take: BFINAL, BTYPE, HLIT, HDIST, HCLEN, 19 lengths of 3 bits; then 7 bits per code length
HEADER_FIXED_MAX = 3 + 5 + 5 + 4 + 3 * 19


# for the sanitizer build: an undefined-behaviour report ends the program (by default it prints and goes on to exit 0)
SANITIZER_ENV = dict(ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")


def make(tool):
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", os.path.basename(tool))], check=True, stdout=subprocess.DEVNULL, timeout=600)


def run_tool(tool, args, timeout=300):
    """one run of deflate_selftest (either build): exit 0 and not a word on stderr, or the test fails with what it said"""
    p = subprocess.run([tool] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **SANITIZER_ENV),
                       timeout=timeout)
    assert p.returncode == 0 and p.stderr == b"", (os.path.basename(tool), args[0], p.returncode, p.stderr.decode(errors="replace")[-2000:])
    return p.stdout


def host_members(tmp, pieces, mis, tool=TOOL):
    """the members the CPU build writes for `pieces`, each read at misalignment `mis`, in one process"""
    src, lens, out, out_lens = (os.path.join(str(tmp), f"{name}_{mis}") for name in ("pieces", "lengths", "members", "member_lengths"))
    with open(src, "wb") as f:
        f.write(b"".join(pieces))
    with open(lens, "w") as f:
        f.write("".join(f"{len(p)}\n" for p in pieces))
    run_tool(tool, ["batch", src, lens, mis, out, out_lens])
    data, at, members = open(out, "rb").read(), 0, []
    for k in map(int, open(out_lens).read().split()):
        members.append(data[at:at + k])
        at += k
    assert at == len(data) and len(members) == len(pieces)
    return members


@functools.lru_cache(maxsize=None)
def model_of(piece):
    """(tokens, literal/length frequencies, distance frequencies, extra bits) of a piece by the model"""
    tokens = dm.tokens_of(piece)
    return (tokens,) + dm.histograms(tokens)


def code_faults(what, freqs, lengths, limit, lone_ok):
    """a Huffman code of `freqs` limited to `limit` bits: used symbols only, complete, optimal where the optimal tree fits"""
    out = []
    if [bool(f) for f in freqs] != [bool(ln) for ln in lengths]:
        out.append(f"{what}: the symbols with a code are not the symbols used")
    if max(lengths) > limit:
        out.append(f"{what}: a code of {max(lengths)} bits")
    have, full = dr.kraft(lengths, limit)
    used = sum(1 for ln in lengths if ln)
    if have != full and not (lone_ok and used == 1 and max(lengths) == 1):
        out.append(f"{what}: Kraft sum {have} / {full}")
    best, depth = dm.huffman_cost(freqs)
    cost = dm.coded_bits(freqs, lengths)
    if depth <= limit and cost != best:
        out.append(f"{what}: {cost} bits where {best} are the optimum and its tree has {depth} levels")
    if cost < best:
        out.append(f"{what}: {cost} bits, fewer than the optimum {best}")
    if not dm.monotone(freqs, lengths):
        out.append(f"{what}: a more frequent symbol has the longer code")
    return out


@functools.lru_cache(maxsize=None)
def member_faults(piece, member):
    """() or what is wrong with `member` as the writer's member of `piece`; also -> BTYPE and the symbols used, for coverage"""
    out, n, m = [], len(piece), member
    if n == 0:
        return (() if m == tr.EOF_MEMBER else ("an empty piece is not the EOF member",)), None, frozenset(), frozenset()
    if m[:10] != b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" or m[10:16] != b"\x06\x00BC\x02\x00":
        out.append("not the BGZF header")
    if len(m) < 26 or struct.unpack_from("<H", m, 16)[0] != len(m) - 1:
        return tuple(out + ["BSIZE is not the member's length - 1"]), None, frozenset(), frozenset()
    if len(m) > 18 + 5 + n + 8:
        out.append(f"{len(m)} bytes: longer than a stored block makes it")
    if struct.unpack_from("<II", m, len(m) - 8) != (zlib.crc32(piece), n):
        out.append("CRC-32 or ISIZE")
    try:
        if zlib.decompress(m, wbits=31) != piece:
            out.append("zlib inflates it to another text")
    except zlib.error as e:
        out.append(f"zlib: {e}")
    try:
        s = dr.read(m[18:len(m) - 8], max_out=n)
    except dr.DeflateError as e:
        return tuple(out + [f"reader: {e}"]), None, frozenset(), frozenset()
    b = s.blocks[0]
    if len(s.blocks) != 1 or b.final != 1 or b.btype not in (0, 2):
        return tuple(out + [f"{len(s.blocks)} blocks, the first of BTYPE {b.btype}"]), b.btype, frozenset(), frozenset()
    if (s.bits + 7) // 8 != len(m) - 26:
        out.append(f"the block ends at bit {s.bits} of {len(m) - 26} bytes")
    elif s.bits % 8 and m[18 + s.bits // 8] >> (s.bits % 8):
        out.append("padding bits are set")
    tokens, lit_freq, dist_freq, extra = model_of(piece)
    lit_best, lit_depth = dm.huffman_cost(lit_freq)
    dist_best, dist_depth = dm.huffman_cost(dist_freq)
    nlit = max(i for i in range(286) if lit_freq[i]) + 1
    ndist = max([i for i in range(30) if dist_freq[i]], default=0) + 1
    if b.btype == 0:
        if len(m) != 18 + 5 + n + 8:
            out.append("a stored member of another length than 18 + 5 + n + 8")
        if lit_depth <= 15 and dist_depth <= 15:                          # the model can price the dynamic form up to its header
            most = HEADER_FIXED_MAX + 7 * (nlit + ndist) + lit_best + dist_best + extra
            if 5 + n > (most + 7) // 8:
                out.append(f"stored in {5 + n} bytes where a dynamic block takes at most {(most + 7) // 8}")
        return tuple(out), 0, frozenset(), frozenset()
    if (s.bits + 7) // 8 >= 5 + n:
        out.append(f"a dynamic block of {(s.bits + 7) // 8} bytes where a stored one takes {5 + n}")
    if b.tokens != tokens:
        k = next((i for i, (x, y) in enumerate(zip(b.tokens, tokens)) if x != y), min(len(b.tokens), len(tokens)))
        out.append(f"token {k}: {b.tokens[k:k + 2]} where the rules give {tokens[k:k + 2]}")
    if (b.hlit, b.hdist) != (nlit, ndist):
        out.append(f"HLIT / HDIST {b.hlit} / {b.hdist} where {nlit} / {ndist} are the trimmed counts")
    if b.hclen > 4 and b.cl_lens[CL_ORDER[b.hclen - 1]] == 0:
        out.append(f"HCLEN {b.hclen} is not trimmed")
    if any(sym >= 16 for sym, _ in b.cl_syms):
        out.append("a repeat symbol (16 .. 18) in the code lengths")
    if b.hlit == nlit and b.hdist == ndist:
        out += code_faults("literal/length code", lit_freq[:nlit], b.lit_lens, 15, lone_ok=False)
        if any(dist_freq):
            out += code_faults("distance code", dist_freq[:ndist], b.dist_lens, 15, lone_ok=True)
        elif b.dist_lens != [1]:
            out.append(f"no match, and distance code lengths {b.dist_lens}")
        cl_freq = [0] * 19
        for ln in b.lit_lens + b.dist_lens:
            cl_freq[ln] += 1
        if sum(1 for f in cl_freq if f) == 1:                             # a second code that is never sent completes the set
            spare = [i for i in range(19) if b.cl_lens[i] and not cl_freq[i]]
            if len(spare) != 1 or b.cl_lens[spare[0]] != 1:
                out.append(f"one code length in use, and code-length code {b.cl_lens}")
            else:
                cl_freq[spare[0]] = 1
                out += code_faults("code-length code", cl_freq, b.cl_lens, 7, lone_ok=False)
        else:
            out += code_faults("code-length code", cl_freq, b.cl_lens, 7, lone_ok=False)
    lengths = frozenset(ls for ls, d in b.symbols if d is not None)
    return tuple(out), 2, lengths, frozenset(d for _, d in b.symbols if d is not None)


def catalogue_faults(named, members):
    """[(name, fault)] over a whole catalogue, and the BTYPE per name"""
    faults, btype = [], {}
    for (name, piece), m in zip(named, members):
        f, btype[name], _, _ = member_faults(piece, m)
        faults += [(name, x) for x in f]
    return faults, btype
