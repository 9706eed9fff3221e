"""The front-end kernels one against the other, alone on the chip and without a profiler: back-to-back launches on the null stream, wall time
per launch.

    python tools/yuv_kernel_bench.py [--launches 3000] [--rounds 5] [--out profiles/yuv_kernel_bench.json]

Feeds: `bgr` (hp_letterbox_u8c3, resize_u8c3_kernel), `nv12-legacy` / `i420-legacy` (hp_letterbox_yuv420, resize_yuv420_kernel) and every
layout of hp_yuv_image through hp_letterbox_yuv (resize_yuv_planar8 / packed8 / word16_kernel).  Two geometries: the stream's own, 1280 x 720
letter-boxed into 432 x 368 - there a launch lasts about as long as the host needs to issue it, so the figure is an upper bound of the
kernel's duration - and 1280 x 720 -> 2560 x 1440, 23 times the output pixels, where the device time dominates and the per-pixel cost of the
kernels can be compared.  Per feed: the minimum and the median over the rounds of (wall time of N launches + one synchronisation) / N.

`p010-hdr` / `i010-hdr` are the same P010 / I010 surfaces read as PQ frames through hp_letterbox_yuv_hdr (resize_yuv_hdr_kernel), beside
`p010` / `i010` (resize_yuv_word16_kernel) of the same run: `hdr_over_sdr` is the ratio of their medians per geometry, the cost of the 24 table
reads per output pixel.  The placement of the tables follows HP_HDR_TABLES (unset: LDS; `global`: device memory through the cache) and is
recorded; one run per placement, the second restricted to the feeds that matter and merged into the same file:

    python tools/yuv_kernel_bench.py
    HP_HDR_TABLES=global python tools/yuv_kernel_bench.py --only p010,i010,p010-hdr,i010-hdr --merge-key hdr_tables_global
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

SW, SH = 1280, 720
GEOMETRIES = {"1280x720 -> 432x368 letterbox": (432, 368), "1280x720 -> 2560x1440": (2560, 1440)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=3000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_kernel_bench.json"))
    ap.add_argument("--only", default=None, help="comma-separated feeds to run (default: all)")
    ap.add_argument("--merge-key", default=None, help="store this run under that key of the existing --out file instead of replacing the file")
    args = ap.parse_args(argv)
    only = set(args.only.split(",")) if args.only else None

    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    rng = np.random.default_rng(3)
    rec = {"method": f"{args.launches} back-to-back launches on the null stream + hp_device_synchronize, wall time / launches, min and median of {args.rounds} rounds; "
                     "no profiler, nothing else on the device",
           "hdr_tables": "global" if os.environ.get("HP_HDR_TABLES") == "global" else "lds", "us_per_launch": {}, "hdr_over_sdr": {}}
    tonemap = frontend.Tonemap("pq")
    for gname, (dw, dh) in GEOMETRIES.items():
        dst = _lib.DevBuf(dw * dh * 3)
        calls = {}
        bgr = _lib.DevBuf.from_numpy(rng.integers(0, 256, (SH, SW, 3), dtype=np.uint8))
        calls["bgr"] = (L.hp_letterbox_u8c3, (bgr.ptr, SW, SH, SW * 3, dst.ptr, dw, dh, dw * 3, 0, 0, 0, None))
        keep = [bgr]
        for fmt in ("nv12", "i420"):
            src = _lib.DevBuf.from_numpy(rng.integers(0, 256, (SH * 3 // 2, SW), dtype=np.uint8))
            f, y, ys, u, v, uvs = frontend._yuv_planes(fmt, src, SW, SH, None, None)
            calls[fmt + "-legacy"] = (L.hp_letterbox_yuv420, (f, y, ys, u, v, uvs, SW, SH, dst.ptr, dw, dh, dw * 3, 0, 0, 0, None))
            keep.append(src)
        for fmt in _lib.YUV_LAYOUTS:
            n = frontend.yuv_packed_bytes(fmt, SW, SH)
            raw = rng.integers(0, 256, n, dtype=np.uint8)
            bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, fmt, SW, SH), fmt)
            im = frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, SW, SH)
            calls[fmt] = (L.hp_letterbox_yuv, (C.byref(im), dst.ptr, dw, dh, dw * 3, 0, 0, 0, None))
            keep += bufs + [im]
            if _lib.YUV_LAYOUTS[fmt][2] == 2:  # the same surface read as a PQ frame
                calls[fmt + "-hdr"] = (L.hp_letterbox_yuv_hdr, (C.byref(im), tonemap.h, dst.ptr, dw, dh, dw * 3, 0, 0, 0, None))
        out = {}
        for name, (fn, a) in calls.items():
            if only is not None and name not in only:
                continue
            for _ in range(200):
                _lib.check(fn(*a))
            _lib.check(L.hp_device_synchronize())
            per = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(args.launches):
                    fn(*a)
                _lib.check(L.hp_device_synchronize())
                per.append((time.perf_counter() - t0) / args.launches * 1e6)
            out[name] = {"min": round(min(per), 2), "median": round(statistics.median(per), 2)}
            print(f"{gname} {name}: min {out[name]['min']} us, median {out[name]['median']} us", flush=True)
        rec["us_per_launch"][gname] = out
        rec["hdr_over_sdr"][gname] = {f: round(out[f + "-hdr"]["median"] / out[f]["median"], 3) for f in ("p010", "i010") if f in out and f + "-hdr" in out}
        print(f"{gname} hdr over sdr ({rec['hdr_tables']}): {rec['hdr_over_sdr'][gname]}", flush=True)
        del keep
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.merge_key:
        whole = json.load(open(args.out)) if os.path.exists(args.out) else {}
        whole[args.merge_key] = rec
        rec = whole
    json.dump(rec, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
