"""The CLI's --scale_ensemble (examples/cli.cpp): the flag is parsed and refused - malformed lists, a parser other than paf, no room for every pass
of a frame - from the flags alone (CPU); on the GPU it runs in both runtimes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-scale.bin")
MODEL = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "6", "--noimshow"]


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def _run(*args):
    return subprocess.run([CLI_BIN, *args], capture_output=True, text=True, timeout=600)


def test_cli_parses_and_refuses_scale_ensemble():
    _build()
    src = "--source=synthetic:1:64x48"
    for bad in ("", "0", "1.5", "-0.5", "0.5,", ",0.5", "0.5,,0.75", "half", "0.5x", "0.5,0.6,0.7,0.8", "nan"):  # refused before any device is touched
        if bad == "":  # (an empty list is the flag's default: off)
            r = _run(src, "--noimshow", f"--scale_ensemble={bad}", "--saving_yuv=/nonexistent/out.yuv")
            assert r.returncode == 1 and "--scale_ensemble" not in r.stdout and "--saving_yuv" in r.stdout, r.stdout + r.stderr
            continue
        r = _run(src, "--noimshow", f"--scale_ensemble={bad}")
        assert r.returncode == 1 and f"--scale_ensemble={bad}:" in r.stdout and "1 .. 3" in r.stdout, (bad, r.stdout + r.stderr)
    for post in ("ppn", "pifpaf"):
        r = _run(src, "--noimshow", "--scale_ensemble=0.5", f"--post={post}")
        assert r.returncode == 1 and "--scale_ensemble" in r.stdout and f"--post={post}" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--scale_ensemble=0.5,0.75", "--max_batch_size=2")  # 3 passes
    assert r.returncode == 1 and "3 network images" in r.stdout and "--max_batch_size=2" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--scale_ensemble=0.5", "--flip_ensemble", "--max_batch_size=3")  # 2 scales and their flips
    assert r.returncode == 1 and "4 network images" in r.stdout and "flips" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--scale_ensemble=0.5", "--tiles=2x2", "--max_batch_size=6")  # 4 regions x 2 scales
    assert r.returncode == 1 and "8 network images" in r.stdout and "region" in r.stdout, r.stdout + r.stderr
    # accepted forms are parsed; the run is then refused for another reason, still before anything touches a device
    for good in (["--scale_ensemble=0.5"], ["--scale_ensemble", "0.5,0.75,1"], ["--scale_ensemble=1", "--flip_ensemble"]):
        r = _run(src, "--noimshow", *good, "--saving_yuv=/nonexistent/out.yuv")
        assert r.returncode == 1 and "--saving_yuv" in r.stdout and "--scale_ensemble" not in r.stdout, (good, r.stdout + r.stderr)


@pytest.mark.gpu
def test_cli_scale_ensemble_runs(tmp_path):
    _build()
    src = "--source=synthetic:4:320x180"
    runs = [_run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--scale_ensemble=0.5", "--saving_prefix", str(tmp_path / "a")),
            _run(*MODEL, src, "--runtime=stream", "--nokeep_ratio", "--scale_ensemble=0.5", "--saving_prefix", str(tmp_path / "b"))]
    for r in runs:
        assert r.returncode == 0 and "4 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert "--scale_ensemble: every frame runs at 2 scales, batches of up to 3" in runs[0].stdout
