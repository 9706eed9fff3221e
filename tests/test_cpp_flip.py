"""The C++ mirror of the flip ensemble (dnn::tensorrt::set_flip_ensemble, the stream's set_flip_ensemble; tests/cpp/flip_api.cpp) compiles with plain
g++ against include/hyperpose/ and the host entry points agree with loops written in the test program (CPU); on the GPU the engine's ensemble maps
equal hp_flip_merge_host of the plain engine's maps, by memcmp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "flip_api.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "flip_api.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + os.path.join(ROOT, "hyperpose_amd"),
                           "-lhp_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_flip_mirror_compiles_and_host_calls_agree():
    _build()
    out = subprocess.run([BIN, "host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.split()[-1] == "HOST_OK", f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.gpu
def test_engine_ensemble_equals_the_c_abi_merge():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared = out.stdout.split()[-2:]
    assert tag == "OK" and int(compared) == 16
