"""The CLI's --tiles / --tile_overlap / --tile_full (examples/cli.cpp): malformed values are refused from the flags alone (CPU); on the GPU a
1 x 1 tiling writes the pictures of a run without tiling, and a 2 x 2 tiling runs on BGR frames in both runtimes, on a raw NV12 clip and
together with --saving_yuv, whose output keeps the clip's size."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-tiles.bin")
MODEL = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "6", "--noimshow"]


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def _run(*args):
    return subprocess.run([CLI_BIN, *args], capture_output=True, text=True, timeout=600)


def test_cli_parses_and_refuses_tile_flags():
    _build()
    src = "--source=synthetic:1:64x48"
    for bad in (["--tiles=3x"], ["--tiles=0x2"], ["--tiles=x2"], ["--tiles=2x2x2"], ["--tiles", "2y2"], ["--tiles=-1x2"], ["--tiles=9x8"],
                ["--tiles=8x8", "--tile_full"], ["--tiles=2x2", "--tile_overlap=-4"], ["--tile_full"]):
        r = _run(src, "--noimshow", *bad)
        assert r.returncode == 1 and "--tiles" in r.stdout, (bad, r.stdout + r.stderr)
    r = _run(src, "--noimshow", "--max_batch_size=4", "--tiles=2x2", "--tile_full")  # parsed, then refused: 5 regions do not fit a batch of 4
    assert r.returncode == 1 and "5 regions" in r.stdout and "--max_batch_size=4" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cli_tiled_runs(tmp_path):
    from hyperpose_amd import synth
    _build()
    src = "--source=synthetic:3:320x180"
    plain = _run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--saving_prefix", str(tmp_path / "plain"))
    one = _run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--tiles=1x1", "--tile_overlap=0", "--saving_prefix", str(tmp_path / "one"))
    tiled = _run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--tiles", "2x2", "--tile_overlap", "32", "--tile_full", "--saving_prefix", str(tmp_path / "t"))
    stream = _run(*MODEL, src, "--runtime=stream", "--nokeep_ratio", "--tiles", "2x2", "--tile_overlap", "32", "--tile_full", "--saving_prefix", str(tmp_path / "s"))
    for r in (plain, one, tiled, stream):
        assert r.returncode == 0 and "3 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    for i in range(3):  # one tile that is the whole frame is no tiling at all
        assert (tmp_path / f"one_{i}.ppm").read_bytes() == (tmp_path / f"plain_{i}.ppm").read_bytes(), i
        assert (tmp_path / f"t_{i}.ppm").exists() and (tmp_path / f"s_{i}.ppm").exists()
    w, h, n = 320, 180, 2
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=79), n, h, w), "nv12", "bt601", "limited")
    clip = b"".join(np.concatenate([p.view(np.uint8).ravel() for p in f]).tobytes() for f in frames)
    (tmp_path / "clip.yuv").write_bytes(clip)
    r = _run(*MODEL, "--runtime=operator", "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", "--tiles=2x2",
             "--saving_prefix", str(tmp_path / "y"), "--saving_yuv", str(tmp_path / "annotated.yuv"))
    assert r.returncode == 0 and f"{n} annotated nv12 frames appended" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert len((tmp_path / "annotated.yuv").read_bytes()) == len(clip)
