"""The C++ mirror's YUV 4:2:0 overloads (include/hyperpose/utility/data.hpp yuv420_frame, dnn::tensorrt::inference / calibrate) compile
with plain g++ (CPU) and return the maps of the cv::Mat overloads on the converted frames, by memcmp (GPU)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "operator_api_yuv.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "operator_api_yuv.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", BIN])


def test_yuv_mirror_compiles():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_yuv_overloads_equal_mat_overloads():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, compared, threw = out.stdout.split()[-3:]
    assert tag == "OK" and int(compared) == 13 and int(threw) == 1


CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-yuv.bin")


def _build_cli():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), CLI_SRC, "-L" + os.path.join(ROOT, "hyperpose_amd"),
                           "-lhp_hip", "-lpthread", "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def test_cli_knows_the_yuv_flags():
    _build_cli()
    r = subprocess.run([CLI_BIN, "--yuv", "--yuv_w=64", "--yuv_h", "48", "--bogus=1"], capture_output=True, text=True)
    assert r.returncode == 1 and "unknown command line flag 'bogus'" in r.stdout
    r = subprocess.run([CLI_BIN, "--noyuv", "--yuv_w"], capture_output=True, text=True)
    assert r.returncode == 1 and "needs a value" in r.stdout


@pytest.mark.gpu
def test_cli_feeds_yuv_frames(tmp_path):
    """`--yuv` on a synthetic source (frames converted to NV12) and a raw I420 file: both go through inference(std::vector<yuv420_frame>)."""
    import numpy as np
    _build_cli()
    common = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "3", "--noimshow"]
    r = subprocess.run([CLI_BIN, *common, "--source=synthetic:5:200x150", "--yuv", "--saving_prefix", str(tmp_path / "a")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "5 images got processed" in r.stdout
    (tmp_path / "clip.yuv").write_bytes(bytes(160 * 120 * 3 // 2))
    r = subprocess.run([CLI_BIN, *common, "--source", str(tmp_path / "clip.yuv")], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--yuv_w" in r.stdout  # raw video carries no header
    clip = np.random.default_rng(4).integers(0, 256, (4, 120 * 3 // 2, 160), dtype=np.uint8)
    (tmp_path / "clip.yuv").write_bytes(clip.tobytes())
    r = subprocess.run([CLI_BIN, *common, "--source", str(tmp_path / "clip.yuv"), "--yuv_w=160", "--yuv_h", "120", "--runtime=stream",
                        "--saving_prefix", str(tmp_path / "b")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert "4 images got processed" in r.stdout and os.path.exists(str(tmp_path / "b_3.ppm"))
