"""The CLI's --encode_yuv (examples/cli.cpp): refusals from the flags alone (CPU); on the GPU raw BGRA frames go in and come out as NV12 frames an
encoder takes - every frame equal to frontend.rgb_to_yuv_host, then frontend.draw_humans_host with the humans the CLI reports - and an odd-sized PPM
picture comes out as an I420 frame padded to 16, redacted and drawn on."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-encode.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def test_cli_refuses_bad_encode_flags_before_the_device(tmp_path):
    _build()
    out = tmp_path / "a.yuv"
    enc = ["--encode_yuv", str(out)]
    for flags, words in [(["--yuv", *enc], ("--encode_yuv", "--yuv", "--saving_yuv")),
                         (["--source=clip.yuv", "--yuv_w=64", "--yuv_h=48", *enc], ("--encode_yuv", ".yuv", "--saving_yuv")),
                         (["--encode_format=nv21", *enc], ("--encode_format=nv21", "i420|nv12|p010|i010|nv16|i422|yuy2|uyvy|i444")),
                         (["--encode_matrix=bt470", *enc], ("--encode_matrix=bt470", "bt601|bt709|bt2020")),
                         (["--encode_range=pc", *enc], ("--encode_range=pc", "limited|full")),
                         (["--encode_align=0", *enc], ("--encode_align=0", "[1, 256]")),
                         (["--encode_align=257", *enc], ("--encode_align=257", "[1, 256]")),
                         (["--encode_format=i420"], ("--encode_format", "--encode_yuv=<file>")),
                         (["--encode_align=16"], ("--encode_align", "--encode_yuv=<file>")),
                         # what was refused before stays refused, word for word
                         (["--rgb=bgra", "--saving_yuv", str(out), *enc], ("--saving_yuv and --redact write video frames; with --rgb=bgra there is none",)),
                         (["--rgb=bgra", "--redact=head"], ("--saving_yuv and --redact write video frames; with --rgb=bgra there is none "
                                                            "(drawing and redaction have no RGB targets)",)),
                         (["--redact=head"], ("--redact=head redacts the frames of --saving_yuv=<file>; the PPM pictures are not redacted",))]:
        r = subprocess.run([CLI_BIN, "--source=synthetic:2:64x48", "--noimshow", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stdout for w in words), (flags, r.stdout + r.stderr)
        assert "ERROR" in r.stdout and not out.exists()


def _humans_of(path, n):
    from hyperpose_amd import _lib
    records, at, humans = path.read_bytes(), 0, []
    for _ in range(n):
        count = int(np.frombuffer(records, "<i4", 1, at)[0])
        humans.append(np.frombuffer(records, _lib.HUMAN_DTYPE, count, at + 4))
        at += 4 + count * _lib.HUMAN_DTYPE.itemsize
    assert at == len(records)
    return humans


@pytest.mark.gpu
def test_cli_encodes_rgb_frames_and_draws_the_reported_humans(tmp_path):
    from hyperpose_amd import _lib, frontend
    _build()
    _lib.init(0)
    common = ["--model", "builtin:lw_openpose_mobilenet", "--w", "160", "--h=128", "--max_batch_size", "2", "--noimshow", "--runtime=operator",
              "--saving_prefix", str(tmp_path / "p")]

    # (1) two raw BGRA frames -> NV12 (BT.709 limited, the defaults), two made-up humans each
    w, h, n = 96, 64, 2
    frames = np.random.default_rng(5).integers(0, 256, (n, h, w, 4), dtype=np.uint8)
    (tmp_path / "clip.rgb").write_bytes(frames.tobytes())
    out = tmp_path / "out.yuv"
    r = subprocess.run([CLI_BIN, *common, "--source", str(tmp_path / "clip.rgb"), f"--yuv_w={w}", f"--yuv_h={h}", "--rgb=bgra", f"--encode_yuv={out}",
                        "--encode_format=nv12", "--synthetic_humans=2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    got, size = out.read_bytes(), frontend.yuv_packed_bytes("nv12", w, h)
    assert len(got) == n * size
    humans = _humans_of(tmp_path / "out.yuv.humans", n)
    assert all(len(x) >= 2 for x in humans)
    for i in range(n):
        planes = frontend.rgb_to_yuv_host(frames[i], "bgra", "nv12", "bt709", "limited")
        plain = b"".join(p.tobytes() for p in planes)
        frontend.draw_humans_host(planes, humans[i], "nv12", "bt709", "limited", opacity=0.5)  # the CLI's default alpha
        want = b"".join(p.tobytes() for p in planes)
        assert want != plain
        assert got[i * size:(i + 1) * size] == want, f"frame {i} is not the converted input, then drawn on"

    # (2) an odd-sized picture -> I420 padded to 16 (BT.601 full), heads redacted, skeletons on top
    pw, ph = 45, 31
    rgb = np.random.default_rng(6).integers(0, 256, (ph, pw, 3), dtype=np.uint8)
    (tmp_path / "pic.ppm").write_bytes(b"P6\n%d %d\n255\n" % (pw, ph) + rgb.tobytes())
    out2 = tmp_path / "pic.yuv"
    r = subprocess.run([CLI_BIN, *common, "--source", str(tmp_path / "pic.ppm"), f"--encode_yuv={out2}", "--encode_format=i420", "--encode_matrix=bt601",
                        "--encode_range=full", "--encode_align=16", "--redact=head", "--redact_effect=black", "--synthetic_humans=2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    assert frontend.yuv_padded_size("i420", pw, ph, 16) == (48, 32)
    got = out2.read_bytes()
    assert len(got) == frontend.yuv_packed_bytes("i420", 48, 32)
    hs = _humans_of(tmp_path / "pic.yuv.humans", 1)[0].copy()  # normalised to the 45 x 31 picture; the surface is 48 x 32
    hs["parts"]["x"] *= np.float32(pw) / np.float32(48)
    hs["parts"]["y"] *= np.float32(ph) / np.float32(32)
    planes = frontend.rgb_to_yuv_host(np.ascontiguousarray(rgb[..., ::-1]), "bgr24", "i420", "bt601", "full", pad_to=16)
    plain = b"".join(p.tobytes() for p in planes)
    frontend.redact_host(planes, frontend.redact_regions(hs, 48, 32, "head", 1.0), "i420", "bt601", "full", effect="black", cell=16)
    frontend.draw_humans_host(planes, hs, "i420", "bt601", "full", opacity=0.5)
    want = b"".join(p.tobytes() for p in planes)
    assert want != plain and got == want
