"""`bamdepth --bam-gpu` on a machine without a device: the usage line names the mode, `--bam-gpu --depth-gz` is a usage error, the
mode fails with the library's error instead of falling back to the host loader, and the C ABI declares the two entry points behind
it (the mode itself: tests/test_gpu_bamdepth_device.py, the kernels: tests/test_gpu_bam_walk.py)."""
import os
import subprocess

import pytest

from palace_amd import capi, synth

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
    for args in ([], ["--bam-gpu"], ["--bam-gpu", "--depth-gz-gpu"], ["--bam-gpu", "--depth-gz-gpu", "out.gz"]):
        p = run(args)
        assert p.returncode == 1 and p.stdout == b"" and b"[--bam-gpu]" in p.stderr
        assert b"--depth-gz-gpu <out.depth.gz>" in p.stderr and b"--depth-gz <out.depth.gz>" in p.stderr


def test_bam_gpu_with_the_host_only_mode_is_a_usage_error(tmp_path):
    bam, gz = str(tmp_path / "t.bam"), str(tmp_path / "t.depth.gz")
    synth.write_bam(bam, [("c1", 100)], [synth.BamRecord("r1", 0, 0, 10, 60, "5M")])
    p = run(["--bam-gpu", "--depth-gz", gz, bam])
    assert p.returncode == 1 and p.stdout == b"" and b"Usage:" in p.stderr
    assert not os.path.exists(gz) and not os.path.exists(gz + ".tbi")


def test_without_a_device_the_mode_fails_and_does_not_fall_back(tmp_path):
    bam, gz = str(tmp_path / "t.bam"), str(tmp_path / "t.depth.gz")
    synth.write_bam(bam, [("c1", 100)], [synth.BamRecord("r1", 0, 0, 10, 60, "5M")])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    for args in ([bam], ["--per-contig", bam], ["--depth-gz-gpu", gz, bam]):
        p = run(["--bam-gpu"] + args, env=env)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr.startswith(b"bamdepth:") and b"device" in p.stderr.lower() and p.stderr.count(b"\n") == 1
    assert not os.path.exists(gz) and not os.path.exists(gz + ".tbi")


def test_the_abi_declares_the_entry_points():
    names = capi.declared_symbols()
    assert "palace_bam_walk" in names and "palace_bam_match_segments" in names
    assert {"palace_bam_walk", "palace_bam_match_segments", "palace_bam_walk_starts", "palace_bam_walk_scratch_bytes"} <= set(capi._SIGS)
