"""The map view against the only other ways to show a network's maps on a device-resident frame, and against the floor of any whole-picture pass.

    python tools/mapview_bench.py [--calls 2000] [--alt-calls 3] [--rounds 5] [--out profiles/mapview_bench.json]

Per configuration - frame 1920 x 1080 | 3840 x 2160, format bgr | nv12 | p010 | yuy2, maps 46 x 54 cells: 19 channels in MAX mode | 38 channels in
FIELD mode - and per round, first `--calls` back-to-back hp_mapview_draw_* calls on the null stream ending in ONE hp_device_synchronize (wall time /
calls, so a call's figure holds its host share too: the palette, the copy of the tap tables, one asynchronous copy, two launches), then, in the same
round: (a) `--alt-calls` times what the library offered before - hp_memcpy_d2h of the frame and the maps into pinned memory + the host twin
(hp_mapview_draw_*_host, the same picture) + hp_memcpy_h2d of the frame; (b) those copies alone, the floor of ANY host-side painter; (c) `--calls`
back-to-back hipMemcpyAsync device-to-device copies of the frame's bytes + one synchronise, the floor of anything that reads and writes the whole
picture once.  Median (and minimum) over the rounds, and the ratios of the medians.  No profiler; nothing else on the device.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(1920, 1080), (3840, 2160)]
FORMATS = ["bgr", "nv12", "p010", "yuy2"]
MAPS = [("max", 19), ("field", 38)]
MAP_H, MAP_W = 46, 54


def image_at(frontend, _lib, fmt: str, base: int, w: int, h: int):
    """hp_yuv_image of one tightly packed frame at address `base` (host or device)"""
    planes, strides, at = [], [], base
    sample = _lib.YUV_LAYOUTS[fmt][2]
    for rows, cols in frontend.yuv_plane_shapes(fmt, w, h):
        planes.append(at), strides.append(cols * sample)
        at += rows * cols * sample
    return frontend.yuv_image(fmt, planes, strides, w, h, "bt709", "limited")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--alt-calls", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapview_bench.json"))
    args = ap.parse_args(argv)

    import mapview_ref
    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3  # hipMemcpyDeviceToDevice
    rng = np.random.default_rng(3)
    rec = {"method": f"per round: {args.calls} back-to-back hp_mapview_draw_* calls on the null stream + one hp_device_synchronize, wall time / calls; then "
                     f"{args.alt_calls} x (hp_memcpy_d2h of frame and maps into pinned memory + host twin + hp_memcpy_h2d of the frame), and the same for the copies "
                     f"alone, wall time / calls; then {args.calls} back-to-back hipMemcpyAsync device-to-device copies of the frame's bytes + one synchronise; "
                     f"median and min of {args.rounds} rounds; no profiler, nothing else on the device; maps {MAP_H} x {MAP_W}, palette jet, alpha scaled, "
                     f"opacity 0.5, gain 1, cover (1, 0.9375)",
           "us_per_call": {}}
    view = frontend.MapView(MAP_H * MAP_W)
    pal = frontend.map_palette("jet", "scaled")
    pp, op = pal.ctypes.data_as(C.c_void_p), C.c_float(0.5)
    for w, h in SIZES:
        for fmt in FORMATS:
            nbytes = w * h * 3 if fmt == "bgr" else frontend.yuv_packed_bytes(fmt, w, h)
            raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
            dev, other = _lib.DevBuf.from_numpy(raw), _lib.DevBuf(nbytes)
            pinned = C.c_void_p()
            _lib.check(L.hp_malloc_host(C.byref(pinned), C.c_size_t(nbytes)))
            for mode, channels in MAPS:
                maps = mapview_ref.blob_maps(channels, 1, channels, MAP_H, MAP_W)
                dmaps = _lib.DevBuf.from_numpy(maps)
                hmaps = np.empty_like(maps)
                dd = frontend._map_desc(dmaps.ptr.value, maps.shape[1:], 0, mode, None, 1.0, (1.0, 0.9375), 0, None)
                hd = frontend._map_desc(hmaps.ctypes.data, maps.shape[1:], 0, mode, None, 1.0, (1.0, 0.9375), 0, None)
                if fmt == "bgr":
                    def device():
                        return L.hp_mapview_draw_u8c3(view.h, dev.ptr, w, h, w * 3, C.byref(dd), pp, op, None)

                    def host():
                        return L.hp_mapview_draw_u8c3_host(pinned, w, h, w * 3, C.byref(hd), pp, op)
                else:
                    dim, him = image_at(frontend, _lib, fmt, dev.ptr.value, w, h), image_at(frontend, _lib, fmt, pinned.value, w, h)

                    def device():
                        return L.hp_mapview_draw_yuv(view.h, C.byref(dim), C.byref(dd), pp, op, None)

                    def host():
                        return L.hp_mapview_draw_yuv_host(C.byref(him), C.byref(hd), pp, op)

                def copies():
                    _lib.check(L.hp_memcpy_d2h(pinned, dev.ptr, C.c_size_t(nbytes)))
                    _lib.check(L.hp_memcpy_d2h(hmaps.ctypes.data_as(C.c_void_p), dmaps.ptr, C.c_size_t(maps.nbytes)))
                    _lib.check(L.hp_memcpy_h2d(dev.ptr, pinned, C.c_size_t(nbytes)))

                def alternative():
                    _lib.check(L.hp_memcpy_d2h(pinned, dev.ptr, C.c_size_t(nbytes)))
                    _lib.check(L.hp_memcpy_d2h(hmaps.ctypes.data_as(C.c_void_p), dmaps.ptr, C.c_size_t(maps.nbytes)))
                    _lib.check(host())
                    _lib.check(L.hp_memcpy_h2d(dev.ptr, pinned, C.c_size_t(nbytes)))

                for _ in range(100):
                    _lib.check(device())
                _lib.check(L.hp_device_synchronize())
                alternative()
                per, alt, cp, d2d = [], [], [], []
                for _ in range(args.rounds):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        device()
                    _lib.check(L.hp_device_synchronize())
                    per.append((time.perf_counter() - t0) / args.calls * 1e6)
                    t0 = time.perf_counter()
                    for _ in range(args.alt_calls):
                        alternative()
                    alt.append((time.perf_counter() - t0) / args.alt_calls * 1e6)
                    t0 = time.perf_counter()
                    for _ in range(args.alt_calls):
                        copies()
                    cp.append((time.perf_counter() - t0) / args.alt_calls * 1e6)
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        hip.hipMemcpyAsync(other.ptr, dev.ptr, nbytes, D2D, None)
                    _lib.check(L.hp_device_synchronize())
                    d2d.append((time.perf_counter() - t0) / args.calls * 1e6)
                med = statistics.median
                key = f"{w}x{h} {fmt} {mode} {channels} channels"
                rec["us_per_call"][key] = {
                    "frame_bytes": int(nbytes),
                    "device": {"min": round(min(per), 2), "median": round(med(per), 2)},
                    "a_d2h_host_twin_h2d": {"min": round(min(alt), 1), "median": round(med(alt), 1)},
                    "b_the_copies_alone": {"min": round(min(cp), 1), "median": round(med(cp), 1)},
                    "c_device_to_device_copy": {"min": round(min(d2d), 2), "median": round(med(d2d), 2)},
                    "a_over_device": round(med(alt) / med(per), 1), "b_over_device": round(med(cp) / med(per), 1),
                    "device_over_c": round(med(per) / med(d2d), 2),
                    "device_GB_per_s_read_plus_written": round(2 * nbytes / med(per) / 1e3, 1)}
                print(key, json.dumps(rec["us_per_call"][key]), flush=True)
                dmaps.free()
            L.hp_free_host(pinned)
            dev.free(), other.free()
    view.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
