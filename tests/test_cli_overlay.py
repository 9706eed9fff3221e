"""The CLI's --saving_yuv (examples/cli.cpp): a raw NV12 clip goes in, the same clip with the skeletons drawn on the device-resident frames
comes out - same size, and every frame equal to frontend.draw_humans_host on the input frame with the humans the CLI reports (GPU)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-overlay.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def test_cli_refuses_saving_yuv_without_video_frames(tmp_path):
    """--saving_yuv on a BGR source without --yuv is refused from the flags alone (no device needed), and nothing is written"""
    _build()
    out = tmp_path / "a.yuv"
    r = subprocess.run([CLI_BIN, "--source=synthetic:2:64x48", "--noimshow", "--saving_yuv", str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--saving_yuv" in r.stdout and "--yuv" in r.stdout, r.stdout + r.stderr
    assert not out.exists() and not (tmp_path / "a.yuv.humans").exists()


@pytest.mark.gpu
def test_cli_saving_yuv_draws_the_reported_humans(tmp_path):
    from hyperpose_amd import _lib, frontend, synth
    _build()
    w, h, n = 200, 150, 4
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=78), n, h, w), "nv12", "bt601", "limited")
    flat = [np.concatenate([p.view(np.uint8).ravel() for p in f]) for f in frames]
    clip = b"".join(f.tobytes() for f in flat)
    (tmp_path / "clip.yuv").write_bytes(clip)
    out_path = tmp_path / "annotated.yuv"
    r = subprocess.run([CLI_BIN, "--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "3", "--noimshow", "--runtime=operator",
                        "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", "--saving_prefix", str(tmp_path / "p"),
                        "--saving_yuv", str(out_path), "--synthetic_humans=3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert f"{n} annotated nv12 frames appended" in r.stdout and "WARNING: --synthetic_humans=3" in r.stdout
    got = out_path.read_bytes()
    assert len(got) == len(clip)
    records = (tmp_path / "annotated.yuv.humans").read_bytes()
    at, total = 0, 0
    size = len(flat[0])
    for i in range(n):
        count = int(np.frombuffer(records, "<i4", 1, at)[0])
        humans = np.frombuffer(records, _lib.HUMAN_DTYPE, count, at + 4)
        at += 4 + count * _lib.HUMAN_DTYPE.itemsize
        total += count
        want = flat[i].copy()
        frontend.draw_humans_host(frontend.yuv_planes(want, "nv12", w, h), humans, "nv12", opacity=0.5)  # the CLI's default alpha
        assert got[i * size:(i + 1) * size] == want.tobytes(), f"frame {i} ({count} humans) is not the input with those humans drawn"
    assert at == len(records)
    print(f"humans drawn over {n} frames: {total}")
    assert total >= 3 * n and got != clip  # the three stand-in humans per frame (--synthetic_humans) next to whatever the parser found
    assert f"({total} humans" in r.stdout  # the same humans the PPM path reports
    assert (tmp_path / "p_0.ppm").exists()  # the PPM output is still written
