"""The C++ mirror's hyperpose::redact_humans (include/hyperpose/utility/redact.hpp) compiles with plain g++ (CPU) and redacts a device-resident
P010 frame and the same frame in host memory to the same bytes, and a device BGR picture to the bytes of the host BGR twin; a bad cell and a
bad margin throw (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "redact_api.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "redact_api.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_redact_humans_mirror_compiles():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_redact_humans_device_equals_host():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared, threw = out.stdout.split()[-3:]
    assert tag == "OK" and int(compared) == 4 and int(threw) == 2
