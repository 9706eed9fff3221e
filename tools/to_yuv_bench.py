"""hp_rgb_to_yuv against the only other way to get an encoder's frame from a device-resident RGB frame, and against the floor of any pass that moves
the same bytes.

    python tools/to_yuv_bench.py [--calls 500] [--alt-calls 2] [--rounds 5] [--step-timeout 180] [--out profiles/to_yuv_bench.json]

Per configuration - source 1920 x 1080 | 3840 x 2160 in bgra | bgr24, target nv12 | p010 | i420 | yuy2 | i444 at BT.709 limited, padded to a multiple
of 16 (1080 -> 1088) - and per round: first `--calls` back-to-back hp_rgb_to_yuv calls on the null stream ending in ONE hp_device_synchronize (wall
time / calls, so a call's figure holds its host share too: the checks, the coefficient table, one launch); then, in the same round, (a) `--alt-calls`
times what a caller had to do before - hp_memcpy_d2h of the source into pinned memory + the host twin hp_rgb_to_yuv_host + hp_memcpy_h2d of the planes;
(b) `--calls` back-to-back hipMemcpyAsync device-to-device copies of (R + W) / 2 bytes + one synchronise, where R is what the conversion reads and W
what it writes: a copy that reads and writes R + W bytes in all, the floor of anything that moves as much.  Median (and minimum) over the rounds and
the ratios of the medians.  No profiler; nothing else on the device.

Every configuration is measured by a process of its own (`--one`), started by this script under `--step-timeout` seconds; the first one that fails or
runs out of time ends the run, and nothing more is started on the device after it.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(1920, 1080), (3840, 2160)]
SOURCES = ["bgra", "bgr24"]
TARGETS = ["nv12", "p010", "i420", "yuy2", "i444"]
ALIGN = 16


def measure(w: int, h: int, fmt_rgb: str, fmt: str, calls: int, alt_calls: int, rounds: int) -> dict:
    import numpy as np

    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3  # hipMemcpyDeviceToDevice
    pw, ph = frontend.yuv_padded_size(fmt, w, h, ALIGN)
    read, written = frontend.rgb_packed_bytes(fmt_rgb, w, h), frontend.yuv_packed_bytes(fmt, pw, ph)
    sample = _lib.YUV_LAYOUTS[fmt][2]

    def image_at(base: int):
        """hp_yuv_image of one tightly packed frame at address `base` (host or device)"""
        planes, strides, at = [], [], base
        for rows, cols in frontend.yuv_plane_shapes(fmt, pw, ph):
            planes.append(at), strides.append(cols * sample)
            at += rows * cols * sample
        return frontend.yuv_image(fmt, planes, strides, pw, ph, "bt709", "limited")

    raw = np.random.default_rng(3).integers(0, 256, read, dtype=np.uint8)
    src, dst = _lib.DevBuf.from_numpy(raw), _lib.DevBuf(written)
    half = (read + written) // 2
    a, b = _lib.DevBuf(half), _lib.DevBuf(half)
    pin_src, pin_dst = C.c_void_p(), C.c_void_p()
    _lib.check(L.hp_malloc_host(C.byref(pin_src), C.c_size_t(read)))
    _lib.check(L.hp_malloc_host(C.byref(pin_dst), C.c_size_t(written)))
    dsrc, hsrc = frontend.rgb_image(fmt_rgb, src, w, h), frontend.rgb_image(fmt_rgb, pin_src.value, w, h)
    ddst, hdst = image_at(dst.ptr.value), image_at(pin_dst.value)

    def device():
        return L.hp_rgb_to_yuv(C.byref(dsrc), C.byref(ddst), None)

    def alternative():
        _lib.check(L.hp_memcpy_d2h(pin_src, src.ptr, C.c_size_t(read)))
        _lib.check(L.hp_rgb_to_yuv_host(C.byref(hsrc), C.byref(hdst)))
        _lib.check(L.hp_memcpy_h2d(dst.ptr, pin_dst, C.c_size_t(written)))

    for _ in range(50):
        _lib.check(device())
    _lib.check(L.hp_device_synchronize())
    got = dst.to_numpy(np.uint8, (written,))
    alternative()
    same = bool(np.array_equal(got, dst.to_numpy(np.uint8, (written,))))  # the two roads give the same frame
    for _ in range(20):
        hip.hipMemcpyAsync(b.ptr, a.ptr, half, D2D, None)
    _lib.check(L.hp_device_synchronize())
    per, alt, d2d = [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(calls):
            device()
        _lib.check(L.hp_device_synchronize())
        per.append((time.perf_counter() - t0) / calls * 1e6)
        t0 = time.perf_counter()
        for _ in range(alt_calls):
            alternative()
        alt.append((time.perf_counter() - t0) / alt_calls * 1e6)
        t0 = time.perf_counter()
        for _ in range(calls):
            hip.hipMemcpyAsync(b.ptr, a.ptr, half, D2D, None)
        _lib.check(L.hp_device_synchronize())
        d2d.append((time.perf_counter() - t0) / calls * 1e6)
    L.hp_free_host(pin_src), L.hp_free_host(pin_dst)
    med = statistics.median
    return {"output": f"{pw}x{ph}", "bytes_read": int(read), "bytes_written": int(written), "device_equals_host_twin": same,
            "device": {"min": round(min(per), 2), "median": round(med(per), 2)},
            "a_d2h_host_twin_h2d": {"min": round(min(alt), 1), "median": round(med(alt), 1)},
            "b_device_to_device_copy": {"min": round(min(d2d), 2), "median": round(med(d2d), 2)},
            "a_over_device": round(med(alt) / med(per), 1), "device_over_b": round(med(per) / med(d2d), 2),
            "device_GB_per_s_read_plus_written": round((read + written) / med(per) / 1e3, 1)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--alt-calls", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=180)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "to_yuv_bench.json"))
    ap.add_argument("--one", nargs=4, metavar=("W", "H", "SOURCE", "TARGET"), help="measure one configuration in this process and print its record")
    args = ap.parse_args(argv)
    if args.one:
        w, h, fmt_rgb, fmt = int(args.one[0]), int(args.one[1]), args.one[2], args.one[3]
        print("RECORD " + json.dumps(measure(w, h, fmt_rgb, fmt, args.calls, args.alt_calls, args.rounds)), flush=True)
        return 0

    rec = {"method": f"per configuration a process of its own; per round: {args.calls} back-to-back hp_rgb_to_yuv calls on the null stream + one "
                     f"hp_device_synchronize, wall time / calls; then {args.alt_calls} x (hp_memcpy_d2h of the source into pinned memory + hp_rgb_to_yuv_host + "
                     f"hp_memcpy_h2d of the planes), wall time / calls; then {args.calls} back-to-back hipMemcpyAsync device-to-device copies of (bytes_read + "
                     f"bytes_written) / 2 bytes (as much traffic as the conversion's) + one synchronise; median and min of {args.rounds} rounds; no profiler, "
                     f"nothing else on the device; BT.709 limited, tightly packed frames, output padded to a multiple of {ALIGN}",
           "us_per_call": {}}
    for w, h in SIZES:
        for fmt_rgb in SOURCES:
            for fmt in TARGETS:
                key = f"{w}x{h} {fmt_rgb} -> {fmt}"
                cmd = [sys.executable, os.path.abspath(__file__), "--one", str(w), str(h), fmt_rgb, fmt, "--calls", str(args.calls), "--alt-calls",
                       str(args.alt_calls), "--rounds", str(args.rounds)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
                except subprocess.TimeoutExpired:
                    print(f"{key}: no result within {args.step_timeout} s; nothing more is started", flush=True)
                    return 3
                lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RECORD ")]
                if out.returncode != 0 or not lines:
                    print(f"{key}: exit {out.returncode}; nothing more is started\n" + out.stdout[-2000:] + out.stderr[-2000:], flush=True)
                    return 2
                rec["us_per_call"][key] = json.loads(lines[-1][len("RECORD "):])
                print(key, json.dumps(rec["us_per_call"][key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
