"""gzip and BGZF writers for the compressed-FASTQ tests (stdlib only), and the getline model of a FASTQ read set.

BGZF members are written by hand: a gzip header whose FEXTRA holds the `BC` subfield (total member size - 1), raw DEFLATE data,
CRC-32 and ISIZE; a file ends with the 28-byte EOF member (SAM/BAM specification, section 4.1)."""
import struct
import zlib

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def deflate_raw(data: bytes, level: int = 6) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def bgzf_member(data: bytes, level: int = 6) -> bytes:
    assert len(data) <= 65536
    body = deflate_raw(data, level)
    total = 18 + len(body) + 8
    assert total <= 65536
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6) + b"BC" + struct.pack("<HH", 2, total - 1)
    return head + body + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def bgzf(data: bytes, block: int = 65280, level: int = 6, eof: bool = True) -> bytes:
    """`data` as BGZF members of `block` input bytes each (level 0: stored blocks)."""
    out = [bgzf_member(data[i:i + block], level) for i in range(0, len(data), block)]
    return b"".join(out) + (BGZF_EOF if eof else b"")


def gzip_member(data: bytes, level: int = 6, fname: bytes | None = None, comment: bytes | None = None, extra: bytes | None = None,
                hcrc: bool = False) -> bytes:
    """One gzip member with the optional header fields FEXTRA, FNAME, FCOMMENT and FHCRC as asked (RFC 1952)."""
    flg = (4 if extra is not None else 0) | (8 if fname is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    head = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, flg, 0, 0, 3)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        head += fname + b"\0"
    if comment is not None:
        head += comment + b"\0"
    if hcrc:
        head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return head + deflate_raw(data, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def gzip_wrap(raw: bytes, text: bytes, fname: bytes | None = None) -> bytes:
    """One gzip member around raw DEFLATE data made elsewhere (tests/deflate_streams.py): header, `raw`, CRC-32 and ISIZE of `text`."""
    head = struct.pack("<BBBBIBB", 0x1F, 0x8B, 8, 8 if fname is not None else 0, 0, 0, 3) + (fname + b"\0" if fname is not None else b"")
    return head + raw + struct.pack("<II", zlib.crc32(text), len(text) & 0xFFFFFFFF)


def gzip_members(data: bytes, cuts, level: int = 6) -> bytes:
    """`data` as several gzip members, cut at the ascending positions `cuts` (anywhere: mid-record, mid-line)."""
    bounds = [0] + [c for c in cuts if 0 < c < len(data)] + [len(data)]
    return b"".join(gzip_member(data[a:b], level) for a, b in zip(bounds, bounds[1:]))


def model_read_set(text: bytes):
    """The reads of FASTQ text as the reference's std::getline loop sees them (extract_ref.cpp:940-1004): lines end at b'\\n'
    only, a last line without one still counts, the empty text behind a final b'\\n' is not a line, sequence lines are the lines
    whose 0-based index is 1 mod 4.  Returns (bases bytes, offsets list)."""
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    seqs = lines[1::4]
    offsets = [0]
    for s in seqs:
        offsets.append(offsets[-1] + len(s))
    return b"".join(seqs), offsets
