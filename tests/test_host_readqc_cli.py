"""`readqc`'s command line where no device is needed or none is visible: usage errors are exit 2 before anything is opened, every fastp
option outside the driver's call is refused by name, and without a device there is a message, a non-zero exit and no file."""
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


def run(args, **kw):
    return subprocess.run([TOOL, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, **kw)


def base_args(d):
    return ["-i", str(d / "r_1.fq"), "-I", str(d / "r_2.fq"), "-o", str(d / "o_1.fq"), "-O", str(d / "o_2.fq")]


def left_behind(d):
    return sorted(p.name for p in d.iterdir() if p.name not in ("r_1.fq", "r_2.fq"))


REFUSED = (["-g"], ["--trim_poly_g"], ["-x"], ["--trim_poly_x"], ["-5"], ["-3"], ["-r"], ["--cut_front"], ["--cut_tail"], ["--cut_right"], ["-c"], ["--correction"],
           ["-U"], ["--umi"], ["-D"], ["--dedup"], ["-m"], ["--merge"], ["-a", "AGATCGGAAGAGC"], ["--adapter_sequence", "AGATCGGAAGAGC"],
           ["--adapter_sequence_r2", "AGATCGGAAGAGC"], ["--detect_adapter_for_pe"], ["-z", "4"], ["--compression", "4"], ["-e", "20"], ["-y"], ["-p"], ["-V"],
           ["--stdout"], ["--interleaved_in"], ["-f", "3"], ["-t", "3"], ["-b", "100"], ["extra.fq"], ["-"], ["--in1"], ["-qq", "3"])


@pytest.mark.parametrize("extra", REFUSED, ids=lambda e: "_".join(e))
def test_options_outside_the_drivers_call_are_usage_errors(files, extra):
    p = run(base_args(files) + extra)
    assert p.returncode == 2 and p.stdout == b"" and b"usage: readqc" in p.stderr and b"readqc: error:" in p.stderr, p.stderr
    assert left_behind(files) == []


def test_required_and_malformed_values(files):
    full = base_args(files)
    for drop in range(0, 8, 2):                                             # each of -i -I -o -O is required: single-end input is not taken
        p = run(full[:drop] + full[drop + 2:])
        assert p.returncode == 2 and b"required" in p.stderr
    for bad in (["-q", "x"], ["-q", "94"], ["-u", "101"], ["-u", "-1"], ["-n", ""], ["-l", "1.5"], ["-w", "many"], ["-q"], ["--length_required=abc"]):
        p = run(full + bad)
        assert p.returncode == 2 and p.stdout == b"", (bad, p.stderr)
    for gz in (["-o", str(files / "o_1.fq.gz")], ["--out2=" + str(files / "o_2.fq.gz")]):
        p = run(full + gz)
        assert p.returncode == 2 and b".gz output" in p.stderr
    assert run([]).returncode == 2
    assert left_behind(files) == []


def test_without_a_device_there_is_a_message_and_no_file(files):
    """every accepted spelling of the driver's call, on a process that sees no device"""
    env = dict(os.environ, ROCR_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    calls = [base_args(files) + ["-w", "8", "-j", str(files / "rep.json"), "-h", str(files / "rep.html")],
             ["--in1", str(files / "r_1.fq"), "--in2=" + str(files / "r_2.fq"), "--out1", str(files / "o_1.fq"), "--out2", str(files / "o_2.fq"), "--thread=4",
              "--json=" + str(files / "rep.json"), "--html", str(files / "rep.html"), "-q", "20", "--unqualified_percent_limit", "30", "--n_base_limit=3",
              "-l", "30", "-A", "--disable_quality_filtering", "-L"]]
    for args in calls:
        for fork in ({}, {"PALACE_NO_FORK": "1"}):
            p = run(args, env=dict(env, **fork))
            assert p.returncode not in (0, 2) and p.stdout == b"", p.stderr
            assert p.stderr.startswith(b"readqc: no GPU device to work on") and b"there is no CPU path" in p.stderr and p.stderr.count(b"\n") == 1, p.stderr
            assert left_behind(files) == []
