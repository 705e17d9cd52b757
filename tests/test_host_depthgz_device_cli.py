"""`bamdepth --depth-gz-gpu` on a machine without a device: the usage line names the mode, and the mode fails with the library's
error instead of falling back to the host path (the mode itself: tests/test_gpu_depthgz_device.py)."""
import os
import subprocess

import pytest

from palace_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAMDEPTH = os.path.join(ROOT, "palace_amd", "bin", "bamdepth")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(os.path.join(ROOT, "palace_amd", "libpalace_hip.so")):
        pytest.skip("libpalace_hip.so not built")
    subprocess.run(["make", "-C", os.path.join(ROOT, "palace_amd", "host"), os.path.join("..", "bin", "bamdepth")], check=True, stdout=subprocess.DEVNULL)


def test_usage_lists_the_mode():
    for args in ([], ["--depth-gz-gpu"], ["--depth-gz-gpu", "out.gz"]):
        p = subprocess.run([BAMDEPTH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode == 1 and b"--depth-gz-gpu <out.depth.gz>" in p.stderr and b"--depth-gz <out.depth.gz>" in p.stderr


def test_without_a_device_the_mode_fails_and_names_it(tmp_path):
    bam, gz = str(tmp_path / "t.bam"), str(tmp_path / "t.depth.gz")
    synth.write_bam(bam, [("c1", 100)], [synth.BamRecord("r1", 0, 0, 10, 60, "5M")])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device, whatever the machine has
    p = subprocess.run([BAMDEPTH, "--depth-gz-gpu", gz, bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 1 and p.stdout == b""
    assert b"bamdepth:" in p.stderr and b"device" in p.stderr.lower()
    assert not os.path.exists(gz)                                                    # nothing was written by another path
