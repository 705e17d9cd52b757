"""The host logic of the device gzip inflater on a CPU (bin/gzip_selftest): DEFLATE block starts from zlib, and the chain walk of
host/gzip_member.hpp over spans of a file -- candidates per stride with false hits among them, member trailers and headers, spans that
end inside blocks -- with zlib standing in for the size pass.  The chunks on the chain must add up to zlib's text member for member."""
import os
import subprocess

import numpy as np

from tests import gz_util as gz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "palace_amd", "bin", "gzip_selftest")


def fastq_like(rng, n):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return b"".join(b"@r%d\n" % i + bytes(rng.choice(acgt, size=100)) + b"\n+\n" + b"I" * 100 + b"\n" for i in range(n))


def test_block_starts_and_chain_walk_against_zlib(tmp_path):
    rng = np.random.default_rng(41)
    text = fastq_like(rng, 30_000)                                   # 6.5 MB
    cases = {
        "one.gz": gz.gzip_member(text, 6),
        "members.gz": gz.gzip_members(text, [len(text) // 3 + 1, len(text) // 2 + 7, len(text) - 5], 1) + gz.gzip_member(text[:200_000], 9, fname=b"x", hcrc=True),
        "stored.gz": gz.gzip_member(text[:300_000], 0),
        "empty_members.gz": gz.gzip_member(b"", 6) + gz.gzip_member(text[:100_000], 6) + gz.gzip_member(b"", 6),
    }
    for name, blob in cases.items():
        p = str(tmp_path / name)
        open(p, "wb").write(blob)
        out = subprocess.run([TOOL, "blocks", p], capture_output=True, text=True)
        assert out.returncode == 0, (name, out.stderr)
        lines = out.stdout.splitlines()
        starts = [int(ln.split()[0]) for ln in lines[:-1]]
        assert starts == sorted(set(starts)) and starts[0] == 80 and lines[-1].startswith(f"blocks {len(starts)} ")
        for stride, span in ((16384, 1 << 30), (1024, len(blob) // 6 + 100), (4096, 150_000), (len(blob) + 5, 1 << 30)):
            span = max(span, 150_000)                                  # a span has to hold more than one block
            if name == "stored.gz":                                    # no dynamic block start to end a span at: one span, one chunk
                span = 1 << 30
            out = subprocess.run([TOOL, "chain", p, str(stride), str(span)], capture_output=True, text=True)
            assert out.returncode == 0 and out.stdout.endswith("chain ok\n"), (name, stride, span, out.stdout, out.stderr)


def test_chain_walk_declines_a_chunk_that_reaches_before_its_member(tmp_path):
    """`chain ... reach`: the size pass also reports how far a chunk's matches reach before its own start, and the walk holds that against
    the member's text so far.  Hand-written streams (tests/deflate_streams.py): the sound ones stay on the chain at every stride and across
    spans, the files whose later chunk reaches before the member's start are declined as PALACE_GZ_MARKER (11) where zlib says
    "invalid distance too far back"."""
    from tests import deflate_streams as ds
    for g in ds.long_streams():
        p = str(tmp_path / (g.name + ".gz"))
        blob = gz.gzip_wrap(g.raw, g.text)
        open(p, "wb").write(blob)
        for stride, span in ((16384, 1 << 30), (512, len(blob) // 4 + 1), (1024, len(blob) // 4 + 1)):
            out = subprocess.run([TOOL, "chain", p, str(stride), str(span), "reach"], capture_output=True, text=True)
            assert out.returncode == 0 and out.stdout.endswith("chain ok\n"), (g.name, stride, span, out.stdout, out.stderr)
            accepted = int(out.stdout.split("accepted ")[1].split()[0])
            assert accepted >= (8 if stride == 16384 else 30), out.stdout
    for name, (blob, _, _) in ds.reach_before_files().items():
        p = str(tmp_path / (name + ".gz"))
        open(p, "wb").write(blob)
        # (the last span ends inside the offending block of the one-member file: the member's text so far is carried into the next span)
        for stride, span in ((16384, 1 << 30), (512, 1 << 30), (512, 17500 if name == "one_member" else 40000)):
            out = subprocess.run([TOOL, "chain", p, str(stride), str(span), "reach"], capture_output=True, text=True)
            assert out.returncode == 1 and out.stdout.startswith("declined: 11 "), (name, stride, span, out.stdout, out.stderr)
            if span == 17500:
                assert out.stdout == "declined: 11 (span 2)\n"
            # without the reach the same walk has nothing to hold against the file: only the CRC would
            out = subprocess.run([TOOL, "chain", p, str(stride), str(span)], capture_output=True, text=True)
            assert out.returncode == 1 and "zlib refuses the file" in out.stderr, (name, stride, out.stdout, out.stderr)
