"""The CLI's --redact (examples/cli.cpp): refusals from the flags alone (CPU); on the GPU a raw NV12 clip goes in and comes out with the persons
redacted on the device-resident frames and the skeletons drawn on top - every frame equal to frontend.redact_host, then
frontend.draw_humans_host, on the input frame with the humans the CLI reports."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-redact.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def test_cli_refuses_bad_redact_flags_before_the_device(tmp_path):
    _build()
    out = tmp_path / "a.yuv"
    video = ["--yuv", "--saving_yuv", str(out)]
    for flags, words in [(["--redact=head"], ("--redact=head", "--saving_yuv")),
                         (["--redact=face", *video], ("--redact=face", "head|body")),
                         (["--redact=body", "--redact_effect=blur", *video], ("--redact_effect=blur", "pixelate|black")),
                         (["--redact=head", "--redact_cell=15", *video], ("--redact_cell=15", "even")),
                         (["--redact=head", "--redact_cell=130", *video], ("--redact_cell=130", "[2, 128]")),
                         (["--redact=head", "--redact_cell=0", *video], ("--redact_cell=0",)),
                         (["--redact=head", "--redact_margin=0", *video], ("--redact_margin=0", "(0, 8]")),
                         (["--redact=head", "--redact_margin=8.5", *video], ("--redact_margin=8.5", "(0, 8]")),
                         (["--redact_only", *video], ("--redact_only", "--redact=head|body")),
                         (["--redact_cell=8", *video], ("--redact_cell", "--redact=head|body"))]:
        r = subprocess.run([CLI_BIN, "--source=synthetic:2:64x48", "--noimshow", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stdout for w in words), (flags, r.stdout + r.stderr)
        assert "ERROR" in r.stdout and not out.exists()


@pytest.mark.gpu
def test_cli_redacts_the_reported_humans_then_draws_them(tmp_path):
    from hyperpose_amd import _lib, frontend, synth
    _build()
    w, h, n = 200, 150, 4
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=78), n, h, w), "nv12", "bt601", "limited")
    flat = [np.concatenate([p.view(np.uint8).ravel() for p in f]) for f in frames]
    clip = b"".join(f.tobytes() for f in flat)
    (tmp_path / "clip.yuv").write_bytes(clip)
    size = len(flat[0])

    def cli(name, *flags):
        out_path = tmp_path / name
        r = subprocess.run([CLI_BIN, "--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "3", "--noimshow", "--runtime=operator",
                            "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", "--saving_prefix", str(tmp_path / "p"),
                            "--saving_yuv", str(out_path), "--synthetic_humans=3", *flags], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        got = out_path.read_bytes()
        assert len(got) == len(clip)
        records, at, humans = (tmp_path / (name + ".humans")).read_bytes(), 0, []
        for _ in range(n):
            count = int(np.frombuffer(records, "<i4", 1, at)[0])
            humans.append(np.frombuffer(records, _lib.HUMAN_DTYPE, count, at + 4))
            at += 4 + count * _lib.HUMAN_DTYPE.itemsize
        assert at == len(records) and sum(len(x) for x in humans) >= 3 * n
        return got, humans

    def expect(humans, what, effect, cell, margin, draw):
        out = []
        for i in range(n):
            want = flat[i].copy()
            planes = frontend.yuv_planes(want, "nv12", w, h)
            frontend.redact_host(planes, frontend.redact_regions(humans[i], w, h, what, margin), "nv12", effect=effect, cell=cell)
            if draw:
                frontend.draw_humans_host(planes, humans[i], "nv12", opacity=0.5)  # the CLI's default alpha
            out.append(want.tobytes())
        return out

    plain, _ = cli("plain.yuv")
    got, humans = cli("heads.yuv", "--redact=head")
    for i, want in enumerate(expect(humans, "head", "pixelate", 16, 1.0, True)):
        assert got[i * size:(i + 1) * size] == want, f"frame {i} is not the input redacted, then drawn on"
    assert got != plain and got != clip
    only, humans = cli("bodies.yuv", "--redact=body", "--redact_effect=black", "--redact_cell=6", "--redact_margin=0.5", "--redact_only")
    for i, want in enumerate(expect(humans, "body", "black", 6, 0.5, False)):
        assert only[i * size:(i + 1) * size] == want, f"frame {i} is not the input redacted"
    assert only != plain and only != got and only != clip
