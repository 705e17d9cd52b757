"""`generateGraph --bam-gpu` as far as it can be judged without a device: the option is there and named by the usage text, it does not
go with --debug, it never falls back to the host loader when no device is visible, and the C ABI it rests on (palace_bam_columns,
palace_bam_name_keys, palace_bam_sa_items, palace_bam_names_differ) is declared and has its ctypes signatures.  What the mode computes:
tests/test_gpu_bam_columns.py (the kernels) and tests/test_gpu_generategraph_device.py (the executable)."""
import os
import subprocess

import pytest

from palace_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
GENERATE_GRAPH = os.path.join(ROOT, "palace_amd", "bin", "generateGraph")
NEW_SYMBOLS = ("palace_bam_columns", "palace_bam_name_keys", "palace_bam_sa_items", "palace_bam_names_differ")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "generateGraph")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture()
def sample(tmp_path):
    targets = [("ctg_a", 2000), ("ctg_b", 1500)]
    recs = [synth.BamRecord(f"r{k}", 0, k % 2, 10 * k, 60, "50M") for k in range(20)]
    bam, fai, out = str(tmp_path / "t.bam"), str(tmp_path / "g.fastg.fai"), str(tmp_path / "graph.txt")
    synth.write_bam(bam, targets, recs)
    open(fai, "w").write("ctg_a:ctg_b;\t2000\t0\t60\t61\n")
    return bam, fai, out


def run(args, **env):
    return subprocess.run([GENERATE_GRAPH] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env), timeout=120)


def own_lines(stderr):
    """stderr without the line the GPU machines' libdrm writes when its ids file is missing"""
    return [l for l in stderr.decode().splitlines() if not l.startswith("/opt/amdgpu/")]


def test_usage_names_the_option():
    p = run([])
    assert p.returncode == 1 and "--bam-gpu" in p.stderr.decode()


def test_debug_is_a_usage_error(sample):
    bam, fai, out = sample
    for args in (["--bam-gpu", "--debug", bam, fai, out, "1"], [bam, "--debug", fai, out, "1", "--bam-gpu"]):      # anywhere getopt takes it
        p = run(args)
        lines = own_lines(p.stderr)
        assert p.returncode == 1 and p.stdout == b"" and len(lines) == 1 and lines[0].startswith("generateGraph:") and "--bam-gpu" in lines[0]
        assert not os.path.exists(out)


@pytest.mark.parametrize("depth", ["1", "auto"])
def test_without_a_device_it_fails_and_never_falls_back(sample, depth):
    bam, fai, out = sample
    p = run(["--bam-gpu", "--min-count", "1", bam, fai, out, depth], HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    lines = own_lines(p.stderr)
    assert p.returncode == 1 and p.stdout == b""
    assert len(lines) == 1 and lines[0].startswith("generateGraph:"), p.stderr
    assert not os.path.exists(out)


def test_the_new_entry_points_are_declared_and_have_signatures():
    declared = capi.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and name in capi._SIGS
