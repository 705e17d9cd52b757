"""`bamdepth --from-depth` on a machine without a device: the usage line names the mode, it goes with no other mode, it fails with
the library's error instead of parsing on the host, and the C ABI declares the two entry points behind it (the mode itself:
tests/test_gpu_bamdepth_from_depth.py, the kernels: tests/test_gpu_depth_parse.py)."""
import os
import subprocess

import pytest

from palace_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMDEPTH = os.path.join(ROOT, "palace_amd", "bin", "bamdepth")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(os.path.join(ROOT, "palace_amd", "libpalace_hip.so")):
        pytest.skip("libpalace_hip.so not built")
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host"), os.path.join("..", "bin", "bamdepth")], check=True, stdout=subprocess.DEVNULL)


def run(args, env=None):
    return subprocess.run([BAMDEPTH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def test_usage_names_the_mode():
    for args in ([], ["--from-depth"], ["--from-depth", "--per-contig"], ["--from-depth", "a", "b"]):
        p = run(args)
        assert p.returncode == 1 and p.stdout == b"" and b"--from-depth [--per-contig] <depth file>" in p.stderr
        assert b"[--bam-gpu]" in p.stderr and b"--depth-gz-gpu <out.depth.gz>" in p.stderr and b"--depth-gz <out.depth.gz>" in p.stderr


def test_with_another_mode_it_is_a_usage_error(tmp_path):
    depth, gz = tmp_path / "t.depth", str(tmp_path / "o.depth.gz")
    depth.write_bytes(b"c1\t1\t1\n")
    for args in (["--bam-gpu", str(depth)], ["--depth-gz", gz, str(depth)], ["--depth-gz-gpu", gz, str(depth)], ["--bam-gpu"],
                 ["--per-contig", "--depth-gz-gpu", gz, str(depth)]):
        p = run(["--from-depth"] + args)
        assert p.returncode == 1 and p.stdout == b"" and b"Usage:" in p.stderr, args
    assert not os.path.exists(gz) and not os.path.exists(gz + ".tbi")


def test_without_a_device_the_mode_fails_and_does_not_fall_back(tmp_path):
    depth = tmp_path / "t.depth"
    depth.write_bytes(b"c1\t1\t1\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    for args in ([str(depth)], ["--per-contig", str(depth)]):
        p = run(["--from-depth"] + args, env=env)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.startswith(b"bamdepth:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1


def test_the_abi_declares_the_entry_points():
    names = capi.declared_symbols()
    assert "palace_depth_parse" in names and "palace_depth_parse_scratch_bytes" in names
    assert {"palace_depth_parse", "palace_depth_parse_scratch_bytes"} <= set(capi._SIGS)
