"""The CLI's --flip_ensemble (examples/cli.cpp): the flag is parsed and refused with a parser other than paf, or without room for a frame and its
flip, from the flags alone (CPU); on the GPU it runs in both runtimes, with --tiles, --rotate and a raw NV12 clip."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-flip.bin")
MODEL = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "6", "--noimshow"]


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def _run(*args):
    return subprocess.run([CLI_BIN, *args], capture_output=True, text=True, timeout=600)


def test_cli_parses_and_refuses_flip_ensemble():
    _build()
    src = "--source=synthetic:1:64x48"
    for post in ("ppn", "pifpaf", "nonsense"):  # refused from the flags alone, before anything touches a device
        r = _run(src, "--noimshow", "--flip_ensemble", f"--post={post}")
        assert r.returncode == 1 and "--flip_ensemble" in r.stdout and f"--post={post}" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--flip_ensemble", "--max_batch_size=1")
    assert r.returncode == 1 and "--flip_ensemble" in r.stdout and "--max_batch_size=1" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--flip_ensemble", "--tiles=2x2", "--max_batch_size=6")  # 4 regions and their flips
    assert r.returncode == 1 and "--flip_ensemble" in r.stdout and "8 network images" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--flip_ensemble=maybe", "--post=ppn", "--saving_yuv=/nonexistent/out.yuv")  # (a value other than true / 1 / yes is false)
    assert r.returncode == 1 and "--flip_ensemble" not in r.stdout and "--saving_yuv" in r.stdout
    # accepted forms are parsed; the run is then refused for another reason, still before anything touches a device
    for good in (["--flip_ensemble"], ["--flip_ensemble=true"], ["-flip_ensemble"], ["--noflip_ensemble", "--post=ppn"], ["--flip_ensemble", "--post", "paf"]):
        r = _run(src, "--noimshow", *good, "--saving_yuv=/nonexistent/out.yuv")
        assert r.returncode == 1 and "--saving_yuv" in r.stdout and "--flip_ensemble" not in r.stdout, (good, r.stdout + r.stderr)


@pytest.mark.gpu
def test_cli_flip_ensemble_runs(tmp_path):
    from hyperpose_amd import synth
    _build()
    src = "--source=synthetic:4:320x180"
    runs = [_run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--flip_ensemble", "--saving_prefix", str(tmp_path / "a")),
            _run(*MODEL, src, "--runtime=stream", "--nokeep_ratio", "--flip_ensemble", "--rotate=90", "--saving_prefix", str(tmp_path / "b")),
            _run(*MODEL, src, "--runtime=operator", "--flip_ensemble", "--tiles=2x1", "--tile_overlap=32", "--half", "--saving_prefix", str(tmp_path / "c")),
            _run(*MODEL, src, "--runtime=stream", "--keep_ratio", "--flip_ensemble", "--tiles=2x1", "--hflip", "--saving_prefix", str(tmp_path / "d"))]
    for r in runs:
        assert r.returncode == 0 and "4 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert "--flip_ensemble: every frame runs with its left-right flip, batches of up to 3" in runs[0].stdout
    w, h, n = 320, 180, 2
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=82), n, h, w), "nv12", "bt601", "limited")
    (tmp_path / "clip.yuv").write_bytes(b"".join(np.concatenate([p.view(np.uint8).ravel() for p in f]).tobytes() for f in frames))
    r = _run(*MODEL, "--runtime=operator", "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", "--flip_ensemble",
             "--saving_prefix", str(tmp_path / "y"))
    assert r.returncode == 0 and f"{n} images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
