"""host/device_scope.hpp, host/mapped_file.hpp, the arithmetic of host/bgzf_members_device.hpp and the BGZF batch reader of
host/bgzf_read_device.hpp -- the device plumbing every host executable shares -- driven by the stand-alone `device_scope_selftest`, as built and under ASan + UBSan.  The program links no
libpalace_hip.so: the library calls the headers make are stubs of its own that count calls, remember what is live and fail on demand
(the cases are listed in palace_amd/host/device_scope_selftest_main.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "palace_amd", "host")
BIN = os.path.join(ROOT, "palace_amd", "bin")
NAMES = ("device_scope_selftest", "device_scope_selftest_asan")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", HOST] + [os.path.join("..", "bin", t) for t in NAMES], check=True, stdout=subprocess.DEVNULL)


@pytest.mark.parametrize("name", NAMES, ids=["plain", "asan"])
def test_selftest(name, tmp_path):
    p = subprocess.run([os.path.join(BIN, name), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = p.stdout.decode().split("\n")
    assert p.returncode == 0 and p.stderr == b"", (p.stdout[-2000:], p.stderr[-2000:])          # (a sanitizer's report goes to stderr)
    assert len(out) == 2 and out[0].startswith("ok ") and int(out[0][3:]) >= 300, out


def test_selftest_does_not_link_the_device_library():
    p = subprocess.run(["ldd", os.path.join(BIN, NAMES[0])], stdout=subprocess.PIPE, check=True)
    assert b"libpalace_hip" not in p.stdout and b"libamdhip64" not in p.stdout


def test_usage():
    p = subprocess.run([os.path.join(BIN, NAMES[0])], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 2 and p.stderr.startswith(b"usage: device_scope_selftest")
