"""What reading a frame upright costs inside the fused resize, alone on the chip and without a profiler: the method of tools/yuv_kernel_bench.py
(back-to-back launches on the null stream, wall time per launch, min and median of the rounds).

    python tools/orientation_bench.py [--launches 3000] [--rounds 5] [--out profiles/orientation_bench.json]

Feeds: bgr, nv12, yuy2, p010-hdr (P010 read as a PQ frame) through hp_resize_oriented_*; codes 0 (the identity: it forwards to the un-oriented
call, so it is the parent kernel and the yardstick OF THE SAME RUN), 1 (a quarter turn), 2 (a half turn), 4 (a mirror).  Two geometries: 1280 x 720
letter-boxed into 432 x 368 - launch-bound, an upper bound only - and 1280 x 720 -> 2560 x 1440, where device time dominates; for a turned frame
"1280 x 720" is the STORED size and the output keeps its size, so every code writes the same number of pixels.  Plus one 3840 x 2160 NV12 frame
into 4 upright regions through hp_resize_rois_oriented_yuv.

Both thread maps of the per-frame kernels (resize_oriented_device.hpp) are measured: the tool runs itself once per map in a child process with
HP_ORIENT_MAP=rows / cols (the library reads it once), and writes both columns, each code as a ratio to code 0 of its own run, and the spread
of code 0 (max - min over the rounds) beside them.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SW, SH = 1280, 720
GEOMETRIES = {"1280x720 -> 432x368 letterbox": (432, 368, 1), "1280x720 -> 2560x1440": (2560, 1440, 0)}
CODES = [0, 1, 2, 4]
FEEDS = ["bgr", "nv12", "yuy2", "p010-hdr"]


def _time(L, check, fn, a, launches, rounds):
    for _ in range(200):
        check(fn(*a))
    check(L.hp_device_synchronize())
    per = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(launches):
            fn(*a)
        check(L.hp_device_synchronize())
        per.append((time.perf_counter() - t0) / launches * 1e6)
    return {"min": round(min(per), 2), "median": round(statistics.median(per), 2), "spread": round(max(per) - min(per), 2)}


def child(args) -> int:
    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    rng = np.random.default_rng(3)
    tonemap = frontend.Tonemap("pq")
    rec = {"us_per_launch": {}}
    srcs, keep = {}, []
    bgr = _lib.DevBuf.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8))
    keep.append(bgr)
    for feed in FEEDS[1:]:
        fmt = feed.split("-")[0]
        raw = rng.integers(0, 256, frontend.yuv_packed_bytes(fmt, SW, SH), dtype=np.uint8)
        bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, fmt, SW, SH), fmt)
        srcs[feed] = frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, SW, SH, "bt2020" if feed.endswith("hdr") else "bt709")
        keep += bufs
    for gname, (w, h, keep_ratio) in GEOMETRIES.items():
        dst = _lib.DevBuf(w * h * 3)
        out = {}
        for feed in FEEDS:
            for code in CODES:
                dw, dh = (h, w) if code & 1 and not keep_ratio else (w, h)  # stretched: the output is turned with the picture
                if feed == "bgr":
                    fn, a = L.hp_resize_oriented_u8c3, (bgr.ptr, SW, SH, SW * 3, code, keep_ratio, 0, 0, 0, dst.ptr, dw, dh, dw * 3, None)
                else:
                    fn, a = L.hp_resize_oriented_yuv, (C.byref(srcs[feed]), tonemap.h if feed.endswith("hdr") else None, code, keep_ratio, 0, 0, 0, dst.ptr,
                                                       dw, dh, dw * 3, None)
                out[f"{feed} code {code}"] = r = _time(L, _lib.check, fn, a, args.launches, args.rounds)
                print(f"[{args.child}] {gname} {feed} code {code}: min {r['min']} us, median {r['median']} us", flush=True)
        rec["us_per_launch"][gname] = out
    # one 4K NV12 frame into 4 upright regions (a 2 x 2 tiling with overlap), each to the network's 432 x 368
    W4, H4 = 3840, 2160
    raw = rng.integers(0, 256, frontend.yuv_packed_bytes("nv12", W4, H4), dtype=np.uint8)
    bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, "nv12", W4, H4), "nv12")
    im = frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, W4, H4, "bt709")
    dst = _lib.DevBuf(4 * 432 * 368 * 3)
    out = {}
    for code in CODES:
        uw, uh = frontend.oriented_size(code, W4, H4)
        rois = frontend.plan_tiles(uw, uh, 2, 2, (64, 64), False, align=(2, 2))
        arr, n = frontend._rois(rois)
        a = (C.byref(im), None, code, arr, n, 1, 0, 0, 0, dst.ptr, 432, 368, 432 * 3, C.c_size_t(432 * 368 * 3), None)
        out[f"nv12 code {code}"] = r = _time(L, _lib.check, L.hp_resize_rois_oriented_yuv, a, args.launches, args.rounds)
        print(f"[{args.child}] 4K rois nv12 code {code}: min {r['min']} us, median {r['median']} us", flush=True)
    rec["us_per_launch"]["3840x2160 nv12 -> 4 regions of 432x368 letterbox (rois call; lanes along rows in both runs)"] = out
    _lib.check(L.hp_device_synchronize())
    tonemap.close()
    json.dump(rec, open(args.child_out, "w"))
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orientation_bench.json"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--child-out", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.child:
        return child(args)
    rec = {"method": f"{args.launches} back-to-back launches on the null stream + hp_device_synchronize, wall time / launches, min, median and spread (max - min) "
                     f"of {args.rounds} rounds; no profiler, nothing else on the device; one child process per thread map (HP_ORIENT_MAP); code 0 forwards "
                     "to the un-oriented call (the parent's kernel) and is the yardstick of its own run",
           "thread_maps": {}, "ratio_to_code_0": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for m in ("rows", "cols"):
            path = os.path.join(tmp, m + ".json")
            env = dict(os.environ, HP_ORIENT_MAP=m)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--launches", str(args.launches), "--rounds", str(args.rounds), "--child", m,
                                   "--child-out", path], env=env)
            rec["thread_maps"][m] = json.load(open(path))["us_per_launch"]
    for m, geoms in rec["thread_maps"].items():
        rec["ratio_to_code_0"][m] = {g: {k: round(v["median"] / out[k.rsplit(" ", 1)[0] + " 0"]["median"], 3) for k, v in out.items()} for g, out in geoms.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec["ratio_to_code_0"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
