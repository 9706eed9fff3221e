"""The C++ mirror of "upright input" (hyperpose::orientation, oriented_size, to_stored / to_upright, draw_humans with an orientation,
dnn::tensorrt::set_orientation; tests/cpp/orientation_api.cpp) compiles with plain g++ against include/hyperpose/ and its host helpers agree with
the C ABI bit for bit (CPU); on the GPU its oriented inference returns the maps of the same calls on host-oriented frames, by memcmp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "orientation_api.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "orientation_api.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + os.path.join(ROOT, "hyperpose_amd"),
                           "-lhp_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_orientation_mirror_compiles_and_agrees_with_the_c_abi():
    _build()
    out = subprocess.run([BIN, "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split()[-1] == "HOST_OK", f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_oriented_inference_equals_inference_of_host_oriented_frames():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared = out.stdout.split()[-2:]
    assert tag == "OK" and int(compared) == 24
