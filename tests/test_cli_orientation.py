"""The CLI's --rotate / --hflip (examples/cli.cpp): values outside 0|90|180|270 are refused from the flags alone (CPU); on the GPU the flags run on
BGR frames in both runtimes, with --tiles, and on a raw NV12 clip with --saving_yuv, whose frames stay in stored orientation with the skeletons of
the recorded UPRIGHT humans drawn through to_stored."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-orientation.bin")
MODEL = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "6", "--noimshow"]


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def _run(*args):
    return subprocess.run([CLI_BIN, *args], capture_output=True, text=True, timeout=600)


def test_cli_parses_and_refuses_orientation_flags():
    _build()
    src = "--source=synthetic:1:64x48"
    for bad in (["--rotate=45"], ["--rotate=-90"], ["--rotate=360"], ["--rotate", "90deg"], ["--rotate="], ["--rotate=1"], ["--rotate=cw"]):
        r = _run(src, "--noimshow", *bad)
        assert r.returncode == 1 and "--rotate" in r.stdout and "0|90|180|270" in r.stdout, (bad, r.stdout + r.stderr)
    r = _run(src, "--noimshow", "--rotate")
    assert r.returncode == 1 and "needs a value" in r.stdout
    # accepted values are parsed; the run is then refused for another reason, still before anything touches a device
    for good in (["--rotate=0"], ["--rotate", "90"], ["--rotate=180", "--hflip"], ["--rotate=270", "--nohflip"], ["--hflip"], ["-rotate=90"]):
        r = _run(src, "--noimshow", *good, "--saving_yuv=/nonexistent/out.yuv")
        assert r.returncode == 1 and "--saving_yuv" in r.stdout and "--rotate" not in r.stdout, (good, r.stdout + r.stderr)


@pytest.mark.gpu
def test_cli_oriented_runs(tmp_path):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import orient_ref
    from hyperpose_amd import _lib, frontend, synth
    _build()
    src = "--source=synthetic:3:320x180"
    runs = [_run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--rotate=90", "--synthetic_humans=2", "--saving_prefix", str(tmp_path / "a")),
            _run(*MODEL, src, "--runtime=stream", "--nokeep_ratio", "--rotate=270", "--hflip", "--saving_prefix", str(tmp_path / "b")),
            _run(*MODEL, src, "--runtime=operator", "--keep_ratio", "--rotate=90", "--tiles=2x2", "--tile_overlap=32", "--saving_prefix", str(tmp_path / "c")),
            _run(*MODEL, src, "--runtime=stream", "--keep_ratio", "--hflip", "--tiles=2x1", "--saving_prefix", str(tmp_path / "d"))]
    for r in runs:
        assert r.returncode == 0 and "3 images got processed" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    for p in "abcd":  # the pictures stay in stored orientation
        assert (tmp_path / f"{p}_0.ppm").read_bytes().startswith(b"P6\n320 180\n")
    w, h, n = 320, 180, 2
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=81), n, h, w), "nv12", "bt601", "limited")
    flat = [np.concatenate([p.view(np.uint8).ravel() for p in f]) for f in frames]
    (tmp_path / "clip.yuv").write_bytes(b"".join(f.tobytes() for f in flat))
    for flags, code in [(["--rotate=90"], 1), (["--rotate=180", "--hflip", "--tiles=2x2"], 6)]:
        r = _run(*MODEL, "--runtime=operator", "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", *flags,
                 "--nokeep_ratio", "--synthetic_humans=2", "--alpha=1", "--saving_prefix", str(tmp_path / "y"), "--saving_yuv", str(tmp_path / "out.yuv"))
        assert r.returncode == 0 and f"{n} annotated nv12 frames appended" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
        written = np.frombuffer((tmp_path / "out.yuv").read_bytes(), np.uint8).reshape(n, -1)
        records = (tmp_path / "out.yuv.humans").read_bytes()
        at = 0
        for i in range(n):
            count = int(np.frombuffer(records, "<i4", 1, at)[0])
            upright = np.frombuffer(records, _lib.HUMAN_DTYPE, count, at + 4)
            at += 4 + count * _lib.HUMAN_DTYPE.itemsize
            assert count >= 2
            assert not np.array_equal(written[i], flat[i]), "nothing was drawn"
            want = [p.copy() for p in frontend.yuv_planes(flat[i], "nv12", w, h)]
            frontend.draw_humans_host(want, orient_ref.humans_orient(upright, code, True), "nv12", "bt601", "limited")
            assert np.array_equal(written[i], np.concatenate([p.ravel() for p in want])), f"{flags}: annotated frame {i} differs"
            as_recorded = [p.copy() for p in frontend.yuv_planes(flat[i], "nv12", w, h)]
            frontend.draw_humans_host(as_recorded, upright, "nv12", "bt601", "limited")
            assert not np.array_equal(written[i], np.concatenate([p.ravel() for p in as_recorded])), "the records were drawn without to_stored"
