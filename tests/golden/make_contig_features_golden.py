"""Writes tests/golden/contig_features_cases.npz: what the reference's encode.matrix_encoding(seq, 3) returns for the seeded
sequences of tests/contig_feature_cases.py.  A generator, not a test:

    python tests/golden/make_contig_features_golden.py <path to the reference's share/palace/scripts/encode.pyx>

encode.pyx is compiled with Cython in a temporary directory outside the repository; nothing compiled is kept."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SETUP = """
from setuptools import setup, Extension
from Cython.Build import cythonize
import numpy
setup(ext_modules=cythonize([Extension("encode", ["encode.pyx"], include_dirs=[numpy.get_include()])], language_level=3))
"""


def main(pyx: str) -> None:
    from tests import contig_feature_cases as cc
    tmp = tempfile.mkdtemp(prefix="encode_build_")
    try:
        shutil.copy(pyx, os.path.join(tmp, "encode.pyx"))
        with open(os.path.join(tmp, "setup.py"), "w") as f:
            f.write(SETUP)
        subprocess.run([sys.executable, "setup.py", "-q", "build_ext", "--inplace"], cwd=tmp, check=True)
        sys.path.insert(0, tmp)
        import encode
        seqs = cc.golden_sequences()
        assert all(len(s) > 0 and not any(48 <= b <= 57 for b in s) for s in seqs)
        out = {"n": np.array(len(seqs))}
        for k, s in enumerate(seqs):
            out["seq_%02d" % k] = np.frombuffer(s, np.uint8)
            out["feat_%02d" % k] = np.asarray(encode.matrix_encoding(s.decode("ascii"), 3), np.float64)
        path = os.path.join(HERE, "contig_features_cases.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes,", len(seqs), "sequences")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main(sys.argv[1])
