"""GPU: the map view on what an engine really produced.  builtin lw_openpose_mobilenet at 160 x 128, batch 2, letter-boxed 200 x 150 NV12 frames:
frontend.draw_maps reads the engine's device output for frame 1 where it lies, on the engine's stream, and the result equals frontend.draw_maps_host
on hp_engine_output_to_host of the same output with the cover from frontend.map_cover - byte for byte."""
import numpy as np
import pytest

from hyperpose_amd import _lib, frontend, synth
from hyperpose_amd.engine import Engine, Model

pytestmark = pytest.mark.gpu
NET_W, NET_H, W, H, PAD = 160, 128, 200, 150, 10


@pytest.mark.parametrize("name,mode,channels", [("conf", "max", 19), ("paf", "field", 38)])
def test_draw_maps_reads_the_engine_output_on_the_device(hp, name, mode, channels):
    from hyperpose_amd import engine as E
    m = Model("lw_openpose_mobilenet", NET_W, NET_H)
    weights = m.init_weights(11)
    for L in m.layers:  # blow up the two output convolutions: random weights then give O(1) maps (tests/test_pipeline_gpu.py)
        if L.op == E.OP_CONV and L.cout in (19, 38) and L.out in [o.tensor for o in m.outputs]:
            weights[L.w_off:L.w_off + L.cout * L.cin] *= 400.0
    engine = Engine.from_model(m, weights, max_batch=2, dtype="f32")
    frames = synth.bgr_to_yuv(synth.images_u8(synth.rng_for(1, salt=78), 2, H, W), "nv12", "bt601", "limited")
    slots = _lib.DevBuf(2 * NET_W * NET_H * 3)
    uploaded = []
    for i, planes in enumerate(frames):
        bufs, strides = frontend.yuv_upload(planes, "nv12", pitch=PAD)
        im = frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, W, H)
        frontend.resize_yuv(im, slots.ptr.value + i * NET_W * NET_H * 3, NET_W, NET_H, keep_ratio=True)
        uploaded.append((bufs, strides, im))
    _lib.check(_lib.lib().hp_device_synchronize())
    engine.enqueue_u8(slots, 2, stream=engine.stream)

    which = [i for i, (_, shape, _) in enumerate(engine.outputs) if shape[0] == channels]
    assert len(which) == 1, [o[:2] for o in engine.outputs]
    dev, shape = engine.output_device(which[0])
    cover = frontend.map_cover(W, H, NET_W, NET_H, True)
    assert cover == (1.0, 120 / 128)
    bufs, strides, im = uploaded[1]
    # the gain is chosen from the maps themselves, so that the view neither saturates nor stays dark: the 90th percentile of what rule 1 reduces lands on 1
    engine.synchronize()
    maps = engine.output_to_host(which[0], 2)
    assert maps.shape == (2,) + tuple(shape) and np.isfinite(maps).all() and not np.array_equal(maps[0], maps[1])
    reduced = np.maximum(maps[1].max(axis=0), 0) if mode == "max" else np.hypot(maps[1][0::2], maps[1][1::2]).max(axis=0)
    gain = float(np.float32(1.0 / np.percentile(reduced, 90)))
    kw = dict(mode=mode, palette=frontend.map_palette("jet", "scaled"), opacity=0.75, gain=gain, cover=cover)
    frontend.draw_maps(im, dev, shape, frame=1, stream=engine.stream, **kw)  # reads the engine's output where it lies
    engine.synchronize()

    want = [np.full((p.shape[0], s), 0xA5, np.uint8) for p, s in zip(frames[1], strides)]
    views = [b[:, :p.shape[1]] for b, p in zip(want, frames[1])]
    for v, p in zip(views, frames[1]):
        v[...] = p
    before = [b.copy() for b in want]
    frontend.draw_maps_host(views, maps, "nv12", index=1, **kw)
    got = [b.to_numpy(np.uint8, w.shape) for b, w in zip(bufs, want)]
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"plane {k}: {len(bad)} bytes differ, first at {bad[0].tolist()}"
    assert any(not np.array_equal(w, b) for w, b in zip(want, before)), "the maps paint nothing"
    plane = frontend.map_index_host(maps, 1, mode, None, gain)
    assert len(np.unique(plane)) > 8, "the view of these maps is nearly flat"
