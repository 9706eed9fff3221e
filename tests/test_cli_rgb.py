"""The CLI's --rgb=<layout> and raw .rgb sources (examples/cli.cpp): an unknown name, --rgb with --yuv, and --saving_yuv or --redact with --rgb are
refused from the flags alone (CPU); on the GPU --rgb=bgra and --rgb=rgb24 report the humans and write the pictures of the plain run, and a raw .rgb
clip gives what its pictures give as PPM files."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgb_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-rgb.bin")
MODEL = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "3", "--noimshow"]


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def _run(*args):
    return subprocess.run([CLI_BIN, *args], capture_output=True, text=True, timeout=600)


def test_cli_refuses_from_the_flags_alone():
    _build()
    src = "--source=synthetic:1:64x48"
    r = _run(src, "--noimshow", "--rgb=bgrx")
    assert r.returncode == 1 and "--rgb=bgrx is not one of rgb24|bgr24|bgra|rgba|argb|abgr|gray" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--rgb=bgra", "--yuv")
    assert r.returncode == 1 and "--rgb=bgra and --yuv" in r.stdout, r.stdout + r.stderr
    r = _run("--source=/nonexistent/clip.yuv", "--noimshow", "--rgb", "gray")
    assert r.returncode == 1 and "--rgb=gray and --yuv" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--rgb=rgb24", "--saving_yuv=/nonexistent/out.yuv")
    assert r.returncode == 1 and "--saving_yuv and --redact" in r.stdout and "--rgb=rgb24" in r.stdout, r.stdout + r.stderr
    r = _run(src, "--noimshow", "--rgb=argb", "--redact=head")
    assert r.returncode == 1 and "--saving_yuv and --redact" in r.stdout and "--rgb=argb" in r.stdout, r.stdout + r.stderr
    r = _run("--source=/nonexistent/clip.rgb", "--noimshow")
    assert r.returncode == 1 and "--rgb=<" in r.stdout, r.stdout + r.stderr


def _outputs(prefix, n):
    return [open(f"{prefix}_{i}.ppm", "rb").read() for i in range(n)]


def _humans(r):
    return int(re.search(r"\((\d+) humans", r.stdout).group(1))


@pytest.mark.gpu
def test_cli_rgb_runs_report_the_humans_of_the_plain_run(tmp_path):
    _build()
    src = "--source=synthetic:5:200x150"
    common = [*MODEL, src, "--runtime=operator", "--keep_ratio", "--synthetic_humans=2"]
    plain = _run(*common, "--saving_prefix", str(tmp_path / "p"))
    assert plain.returncode == 0 and "5 images got processed" in plain.stdout, plain.stdout[-1500:] + plain.stderr[-1500:]
    for layout in ("bgra", "rgb24"):
        r = _run(*common, f"--rgb={layout}", "--saving_prefix", str(tmp_path / layout))
        assert r.returncode == 0 and "5 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        assert _humans(r) == _humans(plain)
        assert _outputs(tmp_path / layout, 5) == _outputs(tmp_path / "p", 5)
    # the other roads run: tiles behind a quarter turn, grey, the stream runtime falling back to the operator one
    r = _run(*MODEL, src, "--rgb=abgr", "--tiles=2x1", "--rotate=90", "--saving_prefix", str(tmp_path / "t"))
    assert r.returncode == 0 and "5 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    r = _run(*MODEL, src, "--rgb=gray", "--runtime=stream", "--saving_prefix", str(tmp_path / "g"))
    assert r.returncode == 0 and "5 images got processed" in r.stdout and "RGB frames go through --runtime=operator" in r.stdout, r.stdout[-1500:]


@pytest.mark.gpu
def test_cli_raw_rgb_source_round_trips(tmp_path):
    _build()
    w, h, n = 120, 90, 3
    rng = np.random.default_rng(8)
    bgr = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    os.mkdir(tmp_path / "pics")
    for i, p in enumerate(bgr):
        (tmp_path / "pics" / f"{i:03d}.ppm").write_bytes(b"P6\n%d %d\n255\n" % (w, h) + p[..., ::-1].tobytes())
    (tmp_path / "clip.rgb").write_bytes(b"".join(rgb_ref.from_bgr(p, "argb", rng).tobytes() for p in bgr))
    size = ["--yuv_w", str(w), f"--yuv_h={h}"]
    want = _run(*MODEL, "--source", str(tmp_path / "pics"), "--saving_prefix", str(tmp_path / "a"))
    got = _run(*MODEL, "--source", str(tmp_path / "clip.rgb"), "--rgb=argb", *size, "--saving_prefix", str(tmp_path / "b"))
    for r in (want, got):
        assert r.returncode == 0 and f"{n} images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    assert _humans(got) == _humans(want)
    assert _outputs(tmp_path / "b", n) == _outputs(tmp_path / "a", n)
    r = _run(*MODEL, "--source", str(tmp_path / "clip.rgb"), "--rgb=argb", "--saving_prefix", str(tmp_path / "c"))
    assert r.returncode != 0 and "--yuv_w" in r.stdout  # raw frames carry no header
    r = _run(*MODEL, "--source", str(tmp_path / "clip.rgb"), "--rgb=rgb24", "--yuv_w=121", "--yuv_h=90", "--saving_prefix", str(tmp_path / "d"))
    assert r.returncode != 0 and "not a whole number of rgb24 frames" in r.stdout
