"""A reader of BAM files through their .bai, written from the SAM specification alone (section 4.1 BGZF, 4.2 the BAM record, 5.2 the
BAI layout, 5.3 reg2bins) -- the checker of `bamsort --bai` / `bamsort --index`; the twin of tests/tabix_reader.py, whose BGZF member
reader it uses.  Independent of the writer: nothing here is shared with it.  Test infrastructure."""
import struct

from tests import bam_sort_cases as bc
from tests.tabix_reader import bgzf_members, reg2bins

PSEUDO_BIN = 37450


def read_bai(path):
    t = open(path, "rb").read()
    assert t[:4] == b"BAI\x01"
    n_ref = struct.unpack_from("<i", t, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", t, at)[0]; at += 4
        bins, order = {}, []
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", t, at); at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", t, at + 16 * k) for k in range(n_chunk)]
            order.append(b)
            at += 16 * n_chunk
        n_intv = struct.unpack_from("<i", t, at)[0]; at += 4
        ioff = list(struct.unpack_from(f"<{n_intv}Q", t, at)); at += 8 * n_intv
        refs.append(dict(bins=bins, order=order, ioff=ioff))
    n_no_coor = struct.unpack_from("<Q", t, at)[0] if at + 8 <= len(t) else None
    assert at + (8 if n_no_coor is not None else 0) == len(t)
    return dict(refs=refs, n_no_coor=n_no_coor)


class IndexedBam:
    def __init__(self, bam_path, bai_path=None):
        self.data = open(bam_path, "rb").read()
        self.members = bgzf_members(self.data)                 # every member checked: magic, BC subfield, CRC-32, ISIZE
        self.stream = b"".join(x for _, x in self.members)
        self.start, acc = {}, 0                                # member file offset -> offset of its bytes in the stream
        for off, x in self.members:
            self.start[off] = acc
            acc += len(x)
        self.start.setdefault(len(self.data), acc)             # (a file without EOF member: its end stands for the stream's end)
        d = self.stream
        assert d[:4] == b"BAM\x01"
        l_text = struct.unpack_from("<i", d, 4)[0]
        self.text = d[8:8 + l_text]
        self.n_ref = struct.unpack_from("<i", d, 8 + l_text)[0]
        at, self.targets = 12 + l_text, []
        for _ in range(self.n_ref):
            l = struct.unpack_from("<i", d, at)[0]
            self.targets.append((d[at + 4:at + 4 + l - 1].decode(), struct.unpack_from("<i", d, at + 4 + l)[0]))
            at += 8 + l
        self.first = at
        self.records = []                                      # (stream offset, bytes)
        while at < len(d):
            n = 4 + struct.unpack_from("<I", d, at)[0]
            self.records.append((at, d[at:at + n]))
            at += n
        assert at == len(d)
        self.bai = read_bai(str(bai_path or str(bam_path) + ".bai"))

    def abs(self, voff):
        coff, uoff = voff >> 16, voff & 0xffff
        assert coff in self.start, f"virtual offset {voff:#x} does not name a member"
        return self.start[coff] + uoff

    def voff_is_canonical(self, voff):
        """inside its member, or at the start of one"""
        coff, uoff = voff >> 16, voff & 0xffff
        size = dict((off, len(x)) for off, x in self.members).get(coff, 0)
        return coff in self.start and (uoff < size or uoff == 0)

    def fetch(self, tid, beg, end, use_linear=True):
        """stream offsets of the records of reference `tid` that overlap [beg, end), found the way a reader of the format does: the
        bins of reg2bins, their chunks whose end lies behind the linear index's entry, a seek to each chunk's start, records read up to its end"""
        ref = self.bai["refs"][tid]
        w = beg >> 14
        min_off = 0
        if use_linear and ref["ioff"]:
            min_off = ref["ioff"][w] if w < len(ref["ioff"]) else ref["ioff"][-1]
        chunks = sorted(c for b in reg2bins(beg, end) if b in ref["bins"] and b != PSEUDO_BIN for c in ref["bins"][b] if c[1] > min_off)
        out = []
        for cb, ce in chunks:
            at, stop = self.abs(cb), self.abs(ce)
            while at < stop:
                n = 4 + struct.unpack_from("<I", self.stream, at)[0]
                rec = self.stream[at:at + n]
                f = bc.fields(rec)
                b, e = bc.span(rec)
                if f["tid"] == tid and b < end and e > beg:
                    out.append(at)
                at += n
            assert at == stop, "a chunk ends inside a record"
        assert len(out) == len(set(out))
        return sorted(out)

    def brute(self, tid, beg, end):
        out = []
        for at, rec in self.records:
            if bc.fields(rec)["tid"] == tid:
                b, e = bc.span(rec)
                if b < end and e > beg:
                    out.append(at)
        return out
