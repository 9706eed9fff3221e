"""The C++ mirror's packed RGB / grey frames (include/hyperpose/utility/data.hpp rgb_frame; dnn::tensorrt::inference / calibrate overloads,
hip_stream::push) compile with plain g++ (CPU) and return the packets and poses of the cv::Mat overloads on the frames converted with
hp_rgb_to_bgr_host, by memcmp (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rgb_frames.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "rgb_frames.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_rgb_mirror_compiles():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_rgb_overloads_equal_mat_overloads():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared, threw = out.stdout.split()[-3:]
    # 2 ratios x (7 layouts x 3 + device, oriented frames, oriented regions, flip ensemble) + int8 calibration + the stream;
    # 2 ratios x (two over-size batches + 5 bad descriptions or regions) + uncalibrated int8 + a batch mixing host and device frames
    assert tag == "OK" and int(compared) == 52 and int(threw) == 16
