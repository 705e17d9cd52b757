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
