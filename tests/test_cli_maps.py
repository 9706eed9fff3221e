"""The CLI's --show_maps (examples/cli.cpp): refusals from the flags alone (CPU); on the GPU a raw NV12 clip goes in and comes out with the network's
maps blended into the device-resident frames and the skeletons drawn on top - every frame equal to frontend.draw_maps_host, then
frontend.draw_humans_host, on the input frame, with the maps of an engine built here like the CLI's and the humans the CLI reports."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "examples", "cli.cpp")
CLI_BIN = os.path.join(ROOT, "examples", "hyperpose-cli-maps.bin")


def _build():
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), CLI_SRC,
                           "-L" + os.path.join(ROOT, "hyperpose_amd"), "-lhp_hip", "-lpthread",
                           "-Wl,-rpath," + os.path.join(ROOT, "hyperpose_amd"), "-o", CLI_BIN])


def test_cli_refuses_bad_map_flags_before_the_device(tmp_path):
    _build()
    out = tmp_path / "a.yuv"
    video = ["--yuv", "--saving_yuv", str(out)]
    for flags, words in [(["--show_maps=conf"], ("--show_maps=conf", "--saving_yuv")),
                         (["--show_maps=paf", "--yuv"], ("--show_maps=paf", "--saving_yuv")),
                         (["--show_maps=heat", *video], ("--show_maps=heat", "conf|paf")),
                         (["--show_maps=conf", "--maps_palette=viridis", *video], ("--maps_palette=viridis", "jet|heat|grey")),
                         (["--show_maps=conf", "--maps_alpha=linear", *video], ("--maps_alpha=linear", "constant|scaled")),
                         (["--show_maps=conf", "--maps_opacity=0", *video], ("--maps_opacity=0", "(0, 1]")),
                         (["--show_maps=conf", "--maps_opacity=1.5", *video], ("--maps_opacity=1.5", "(0, 1]")),
                         (["--show_maps=paf", "--runtime=stream", *video], ("--show_maps=paf", "--runtime=stream")),
                         (["--maps_palette=heat", *video], ("--maps_palette", "--show_maps=conf|paf")),
                         (["--maps_opacity=0.25", *video], ("--maps_opacity", "--show_maps=conf|paf"))]:
        r = subprocess.run([CLI_BIN, "--source=synthetic:2:64x48", "--noimshow", *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and all(w in r.stdout for w in words), (flags, r.stdout + r.stderr)
        assert "ERROR" in r.stdout and not out.exists()


@pytest.mark.gpu
def test_cli_shows_the_maps_then_draws_the_reported_humans(tmp_path):
    from hyperpose_amd import _lib, frontend, synth
    from hyperpose_amd.engine import Engine, Model
    _build()
    _lib.init(0)
    w, h, n, net_w, net_h, batch = 200, 150, 4, 160, 128, 3
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=78), n, h, w), "nv12", "bt601", "limited")
    flat = [np.concatenate([p.view(np.uint8).ravel() for p in f]) for f in frames]
    clip = b"".join(f.tobytes() for f in flat)
    (tmp_path / "clip.yuv").write_bytes(clip)
    size = len(flat[0])

    def cli(name, *flags):
        out_path = tmp_path / name
        r = subprocess.run([CLI_BIN, "--model", "builtin:lw_openpose_mobilenet", "--w", str(net_w), f"--h={net_h}", "--max_batch_size", str(batch), "--noimshow",
                            "--runtime=operator", "--source", str(tmp_path / "clip.yuv"), f"--yuv_w={w}", f"--yuv_h={h}", "--yuv_format=nv12", "--saving_prefix",
                            str(tmp_path / "p"), "--saving_yuv", str(out_path), "--synthetic_humans=3", *flags], capture_output=True, text=True, timeout=600)
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

    # the CLI's engine, built here: the same architecture, seed, precision and batch size, fed the same letter-boxed frames in the same batches
    m = Model("lw_openpose_mobilenet", net_w, net_h)
    engine = Engine.from_model(m, m.init_weights(20241), max_batch=batch, dtype="f32")
    slots = _lib.DevBuf(batch * net_w * net_h * 3)
    maps = {19: [], 38: []}
    for first in range(0, n, batch):
        count = min(batch, n - first)
        for k in range(count):
            bufs, strides = frontend.yuv_upload(frames[first + k], "nv12")
            im = frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, w, h)
            frontend.resize_yuv(im, slots.ptr.value + k * net_w * net_h * 3, net_w, net_h, keep_ratio=True)
        _lib.check(_lib.lib().hp_device_synchronize())
        engine.enqueue_u8(slots, count)
        engine.synchronize()
        for i, (_, shape, _) in enumerate(engine.outputs):
            maps[shape[0]] += list(engine.output_to_host(i, count))
    cover = frontend.map_cover(w, h, net_w, net_h, True)

    def expect(humans, channels, mode, palette, alpha, opacity, gain):
        out = []
        for i in range(n):
            want = flat[i].copy()
            planes = frontend.yuv_planes(want, "nv12", w, h)
            frontend.draw_maps_host(planes, maps[channels][i][None], "nv12", mode=mode, palette=frontend.map_palette(palette, alpha), opacity=opacity, gain=gain,
                                    cover=cover)
            frontend.draw_humans_host(planes, humans[i], "nv12", opacity=0.5)  # the CLI's default alpha
            out.append(want.tobytes())
        return out

    # the gains are chosen from the maps (seeded weights give small ones): the 90th percentile of what rule 1 reduces lands on 1.  A float32
    # printed in full goes through the CLI's double and back unchanged
    conf_gain = float(np.float32(1.0 / np.percentile(np.maximum(maps[19][1].max(axis=0), 0), 90)))
    paf_gain = float(np.float32(1.0 / np.percentile(np.hypot(maps[38][1][0::2], maps[38][1][1::2]).max(axis=0), 90)))
    planes = [frontend.map_index_host(maps[c][1][None], 0, mode, None, g) for c, mode, g in ((19, "max", conf_gain), (38, "field", paf_gain))]
    assert all(len(np.unique(p)) > 8 for p in planes), "the views of these maps are nearly flat"

    plain, _ = cli("plain.yuv")
    got, humans = cli("conf.yuv", "--show_maps=conf", f"--maps_gain={conf_gain!r}")
    for i, want in enumerate(expect(humans, 19, "max", "jet", "constant", 0.5, conf_gain)):
        assert got[i * size:(i + 1) * size] == want, f"frame {i} is not the input with its confidence maps, then drawn on"
    assert got != plain and got != clip
    paf, humans = cli("paf.yuv", "--show_maps=paf", f"--maps_gain={paf_gain!r}", "--maps_palette=heat", "--maps_alpha=scaled", "--maps_opacity=0.75")
    for i, want in enumerate(expect(humans, 38, "field", "heat", "scaled", 0.75, paf_gain)):
        assert paf[i * size:(i + 1) * size] == want, f"frame {i} is not the input with its part-affinity fields, then drawn on"
    assert paf != plain and paf != got
