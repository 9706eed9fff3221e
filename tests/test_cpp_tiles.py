"""The C++ mirror of tiled inference (hyperpose::tiling, plan_tiles, to_frame, merge_humans, dnn::tensorrt::inference(frame, regions),
stream::set_tiling) compiles with plain g++; its host half equals the C ABI (CPU) and its engine half equals the per-region inference of
cut-out frames by memcmp (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tiles.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "tiles.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_tiles_mirror_compiles_and_its_host_half_equals_the_c_abi():
    _build()
    out = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.split()[-2:] == ["HOST_OK", "6"]


@pytest.mark.gpu
def test_region_inference_equals_inference_of_the_cut_outs():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared, threw = out.stdout.split()[-3:]
    assert tag == "OK" and int(compared) == 2 * (6 + 5) and int(threw) == 4
