"""`bamsort` on a machine without a device: usage errors, the options of `samtools sort` it does not take, the -O error, the one-line
device error that leaves no file, and the C ABI behind it (the tool itself: tests/test_gpu_bamsort_cli.py, the kernels:
tests/test_gpu_sort_u64.py and tests/test_gpu_bam_sort.py)."""
import os
import subprocess

import pytest

from palace_amd import capi
from tests import gz_util
from tests.test_host_bam_spec import header, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMSORT = os.path.join(ROOT, "palace_amd", "bin", "bamsort")
ENTRY_POINTS = {"palace_bam_sort_keys", "palace_sort_u64_scratch_bytes", "palace_sort_u64", "palace_bam_gather_plan", "palace_bam_gather_write",
                "palace_bai_records", "palace_bai_chunks", "palace_bai_linear", "palace_bgzf_voffsets"}


@pytest.fixture(scope="module", autouse=True)
def built():
    capi.build()
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host"), os.path.join("..", "bin", "bamsort")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture
def bam(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(gz_util.bgzf(header([("c1", 100)]) + record("r1", 0, 0, 10, 60, "5M")))
    return str(path)


def run(args, env=None):
    return subprocess.run([BAMSORT] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120)


def test_usage_errors(tmp_path, bam):
    out = str(tmp_path / "out.bam")
    for args in ([], [bam], ["-o", out], ["-o", out, bam, bam], ["-o"], ["-@", "x", "-o", out, bam], ["-@"], ["-O", "BAM", bam], ["--index"],
                 ["--index", bam, "a.bai", "b.bai"], ["--index", "--bai", bam], ["--bogus", "-o", out, bam]):
        p = run(args)
        assert p.returncode == 1 and p.stdout == b"" and b"Usage: bamsort" in p.stderr and b"--index <sorted.bam>" in p.stderr, args
    assert os.listdir(tmp_path) == ["in.bam"]


def test_the_other_options_of_samtools_sort_are_refused(tmp_path, bam):
    out = str(tmp_path / "out.bam")
    for extra in (["-n"], ["-t", "RG"], ["-m", "1G"], ["-T", str(tmp_path / "tmp")], ["-l", "5"], ["-u"], ["--no-PG"], ["--write-index"]):
        p = run(extra + ["-@", "4", "-O", "BAM", "-o", out, bam])
        assert p.returncode == 1 and p.stdout == b"" and b"Usage: bamsort" in p.stderr, extra
    assert os.listdir(tmp_path) == ["in.bam"]


def test_only_bam_is_written(tmp_path, bam):
    out = str(tmp_path / "out.sam")
    for fmt in ("SAM", "CRAM", "sam"):
        p = run(["-O", fmt, "-o", out, bam])
        assert p.returncode == 1 and p.stdout == b"" and p.stderr.startswith(b"bamsort: -O " + fmt.encode()) and p.stderr.count(b"\n") == 1
    assert os.listdir(tmp_path) == ["in.bam"]


def test_without_a_device_it_fails_with_one_line_and_leaves_no_file(tmp_path, bam):
    out = str(tmp_path / "out.bam")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    for args in (["-@", "4", bam, "-O", "BAM", "-o", out], ["-Obam", "-o" + out, "--bai", bam, "-@2"], ["--index", bam], ["--index", bam, str(tmp_path / "x.bai")]):
        p = run(args, env=env)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.startswith(b"bamsort:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1
    assert os.listdir(tmp_path) == ["in.bam"]


def test_the_abi_declares_the_entry_points():
    assert ENTRY_POINTS <= set(capi.declared_symbols()) and ENTRY_POINTS <= set(capi._SIGS)
    text = open(os.path.join(ROOT, "include", "palace_hip.h")).read()
    assert f"#define PALACE_SORT_TILE {capi.SORT_TILE} " in text
