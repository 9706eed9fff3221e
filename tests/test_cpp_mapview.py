"""The C++ mirror's hyperpose::draw_maps (include/hyperpose/utility/map_view.hpp) compiles with plain g++ (CPU) and paints an engine's maps into a
device-resident P010 frame and the same frame in host memory to the same bytes - from the engine's device output while it is valid and from a staged
copy afterwards - and a turned device BGR picture to the bytes of the host BGR twin; an opacity of 0 throws (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mapview_api.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "mapview_api.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_draw_maps_mirror_compiles():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_draw_maps_device_equals_host():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared, threw = out.stdout.split()[-3:]
    assert tag == "OK" and int(compared) == 6 and int(threw) == 1
