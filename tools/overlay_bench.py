"""The overlay renderer against the only other way to annotate a device-resident frame: copy it to the host, draw there, copy it back.

    python tools/overlay_bench.py [--calls 2000] [--alt-calls 10] [--rounds 5] [--out profiles/overlay_bench.json]

Per configuration - frame 1920 x 1080 | 3840 x 2160, 8 | 32 seeded synthetic humans, format bgr | nv12 | p010 | yuy2 - and per round, first
`--calls` back-to-back hp_overlay_draw_* calls on the null stream ending in ONE hp_device_synchronize (the method of tools/yuv_kernel_bench.py:
wall time / calls, so a call's figure holds its host share too - the primitive list, one small asynchronous copy, the launch), then, in the same
round, `--alt-calls` times the alternative on the same frame: hp_memcpy_d2h of the whole frame into pinned memory + the host twin
(hp_overlay_draw_*_host, the same picture) + hp_memcpy_h2d, and the two copies alone - the floor of ANY host-side rasteriser.  Minimum and median over the rounds of both, and their ratio.  No profiler; nothing
else on the device.  The kernel touches a few hundred KB of a frame and is launch- and latency-bound: no share of any peak is claimed.
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(1920, 1080), (3840, 2160)]
HUMANS = [8, 32]
FORMATS = ["bgr", "nv12", "p010", "yuy2"]


def synthetic_humans(seed: int, n: int):
    """n standing figures, all 18 parts, about a sixth of the frame wide and a third high, centres spread over the frame"""
    from hyperpose_amd import _lib
    r = np.random.default_rng(seed)
    hs = np.zeros(n, _lib.HUMAN_DTYPE)
    for h in hs:
        cx, cy = r.uniform(0.1, 0.9), r.uniform(0.2, 0.8)
        for k in range(18):
            h["parts"][k] = (1, cx + r.uniform(-0.08, 0.08), cy + r.uniform(-0.17, 0.17), 1.0)
        h["score"] = 1.0
    return hs


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
    ap.add_argument("--alt-calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_bench.json"))
    args = ap.parse_args(argv)

    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    rng = np.random.default_rng(3)
    rec = {"method": f"per round: {args.calls} back-to-back hp_overlay_draw_* calls on the null stream + one hp_device_synchronize, wall time / calls; then "
                     f"{args.alt_calls} x (hp_memcpy_d2h of the frame into pinned memory + host twin + hp_memcpy_h2d), wall time / calls, and the same for the two copies alone; min and median of "
                     f"{args.rounds} rounds; no profiler, nothing else on the device; opacity 0.5, thickness by the reference's rule",
           "us_per_call": {}}
    ov = frontend.Overlay(max(HUMANS))
    for w, h in SIZES:
        for fmt in FORMATS:
            nbytes = w * h * 3 if fmt == "bgr" else frontend.yuv_packed_bytes(fmt, w, h)
            raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
            dev = _lib.DevBuf.from_numpy(raw)
            pinned = C.c_void_p()
            _lib.check(L.hp_malloc_host(C.byref(pinned), C.c_size_t(nbytes)))
            for n in HUMANS:
                hs = synthetic_humans(100 + n, n)
                hp = hs.ctypes.data_as(C.c_void_p)
                op = C.c_float(0.5)
                if fmt == "bgr":
                    def device():
                        return L.hp_overlay_draw_u8c3(ov.h, dev.ptr, w, h, w * 3, hp, n, op, 0, None)

                    def host():
                        return L.hp_overlay_draw_u8c3_host(pinned, w, h, w * 3, hp, n, op, 0)
                else:
                    dim, him = image_at(frontend, _lib, fmt, dev.ptr.value, w, h), image_at(frontend, _lib, fmt, pinned.value, w, h)

                    def device():
                        return L.hp_overlay_draw_yuv(ov.h, C.byref(dim), hp, n, op, 0, None)

                    def host():
                        return L.hp_overlay_draw_yuv_host(C.byref(him), hp, n, op, 0)

                def alternative():
                    _lib.check(L.hp_memcpy_d2h(pinned, dev.ptr, C.c_size_t(nbytes)))
                    _lib.check(host())
                    _lib.check(L.hp_memcpy_h2d(dev.ptr, pinned, C.c_size_t(nbytes)))

                def copies():
                    _lib.check(L.hp_memcpy_d2h(pinned, dev.ptr, C.c_size_t(nbytes)))
                    _lib.check(L.hp_memcpy_h2d(dev.ptr, pinned, C.c_size_t(nbytes)))

                for _ in range(100):
                    _lib.check(device())
                _lib.check(L.hp_device_synchronize())
                alternative()
                per, alt, cp = [], [], []
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
                key = f"{w}x{h} {fmt} {n} humans"
                rec["us_per_call"][key] = {
                    "primitives": int(len(frontend.overlay_primitives(hs, w, h))), "frame_bytes": int(nbytes),
                    "device": {"min": round(min(per), 2), "median": round(statistics.median(per), 2)},
                    "d2h_host_h2d": {"min": round(min(alt), 1), "median": round(statistics.median(alt), 1)},
                    "of_which_the_two_copies": {"min": round(min(cp), 1), "median": round(statistics.median(cp), 1)},
                    "ratio_of_medians": round(statistics.median(alt) / statistics.median(per), 1)}
                print(key, json.dumps(rec["us_per_call"][key]), flush=True)
            L.hp_free_host(pinned)
            dev.free()
    ov.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
