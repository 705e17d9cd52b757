"""`readqc --full-report` where no device is needed or none is visible: the option is taken with -j and is a usage error without it,
before anything is opened."""
import os
import subprocess

import pytest

from tests import readqc_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
TOOL = os.path.join(ROOT, "palace_amd", "bin", "readqc")


@pytest.fixture(scope="module", autouse=True)
def built():
    from palace_amd import capi
    capi.build()
    subprocess.run(["make", "-C", HOST, os.path.join("..", "bin", "readqc")], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture()
def files(tmp_path):
    t1, t2 = rc.texts_of([(b"ACGT" * 10, b"I" * 40, b"TTGA" * 10, b"I" * 40)])
    (tmp_path / "r_1.fq").write_bytes(t1)
    (tmp_path / "r_2.fq").write_bytes(t2)
    return tmp_path


def run(d, extra, **kw):
    args = ["-i", str(d / "r_1.fq"), "-I", str(d / "r_2.fq"), "-o", str(d / "o_1.fq"), "-O", str(d / "o_2.fq")] + extra
    return subprocess.run([TOOL, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def left_behind(d):
    return sorted(p.name for p in d.iterdir() if p.name not in ("r_1.fq", "r_2.fq"))


def test_full_report_without_json_is_a_usage_error(files):
    for extra in (["--full-report"], ["--full-report", "-h", str(files / "rep.html")]):
        p = run(files, extra)
        assert p.returncode == 2 and p.stdout == b"" and b"usage: readqc" in p.stderr and b"readqc: error: --full-report needs -j" in p.stderr, p.stderr
        assert left_behind(files) == []
    for extra in (["--full-report=1", "-j", str(files / "rep.json")], ["--full_report", "-j", str(files / "rep.json")]):        # a flag of one spelling
        p = run(files, extra)
        assert p.returncode == 2 and b"is not taken" in p.stderr and left_behind(files) == []


def test_full_report_with_json_goes_on_to_the_device(files):
    env = dict(os.environ, ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    p = run(files, ["-j", str(files / "rep.json"), "--full-report"], env=env)
    assert p.returncode not in (0, 2) and p.stdout == b"" and p.stderr.startswith(b"readqc: no GPU device to work on"), p.stderr
    assert left_behind(files) == []
