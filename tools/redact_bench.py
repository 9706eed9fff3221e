"""Redaction on the device against the only other way to redact a device-resident frame: copy it to the host, redact there, copy it back.

    python tools/redact_bench.py [--calls 1000] [--alt-calls 5] [--rounds 5] [--out profiles/redact_bench.json]

Per configuration - frame 1920 x 1080 | 3840 x 2160, 8 | 32 seeded standing figures in human proportions, heads | bodies, format bgr | nv12 | p010 | yuy2, pixelate,
cell 16 - and per round, first `--calls` back-to-back hp_redact_* calls on the null stream ending in ONE hp_device_synchronize (the method of
tools/overlay_bench.py: wall time / calls, so a call's figure holds its host share too - the region checks, one small asynchronous copy, the
launch), then, in the same round, `--alt-calls` times the detour on the same frame: hp_memcpy_d2h of the whole frame into pinned memory + the
host twin (hp_redact_*_host, the same picture) + hp_memcpy_h2d, and the two copies alone - the floor of ANY host-side redaction.  Minimum and
median over the rounds of both, and their ratio.  Redacting a redacted frame rewrites the same bytes, so every call does the same work.
`hit_cell_bytes` is the size of the samples of the cells the regions reach (numpy, from the rules of DESIGN.md 1.1); a pixelating call reads
and writes each once, and `device_gb_per_s` = 2 * hit_cell_bytes / the median call - a whole-call rate, host share included, not a kernel's
share of any peak.  No profiler; nothing else on the device.
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

from tools.overlay_bench import FORMATS, HUMANS, SIZES, image_at  # noqa: E402

WHAT = ["head", "body"]
CELL = 16
BYTES_PER_PIXEL = {"bgr": 3.0, "nv12": 1.5, "p010": 3.0, "yuy2": 2.0}


# a standing figure in units of its height (x to the figure's left, y down from the top of the head), COCO part order: nose, neck, right
# shoulder / elbow / wrist, left shoulder / elbow / wrist, right hip / knee / ankle, left hip / knee / ankle, right eye, left eye, right ear, left ear
FIGURE = [(0.0, 0.07), (0.0, 0.17), (-0.11, 0.18), (-0.14, 0.34), (-0.15, 0.48), (0.11, 0.18), (0.14, 0.34), (0.15, 0.48), (-0.06, 0.5), (-0.07, 0.74),
          (-0.07, 0.97), (0.06, 0.5), (0.07, 0.74), (0.07, 0.97), (-0.02, 0.055), (0.02, 0.055), (-0.045, 0.065), (0.045, 0.065)]


def standing_humans(seed: int, n: int, w: int, h: int):
    """n standing figures with all 18 parts in human proportions (a head about an eighth of the figure), a third to two thirds of the frame
    high, spread over the frame; a little jitter on every part"""
    from hyperpose_amd import _lib
    r = np.random.default_rng(seed)
    hs = np.zeros(n, _lib.HUMAN_DTYPE)
    for hm in hs:
        tall = r.uniform(0.33, 0.66)  # of the frame's height
        cx, top = r.uniform(0.08, 0.92), r.uniform(0.02, 0.98 - tall)
        for k, (fx, fy) in enumerate(FIGURE):
            hm["parts"][k] = (1, cx + (fx + r.uniform(-0.004, 0.004)) * tall * h / w, top + (fy + r.uniform(-0.004, 0.004)) * tall, 1.0)
        hm["score"] = 1.0
    return hs


def hit_pixels(regions, w: int, h: int, cell: int) -> int:
    """pixels of the cells (clipped to the frame) that any region reaches: the hit test of DESIGN.md 1.1 over the whole cell grid at once"""
    X0, Y0 = np.meshgrid(np.arange(0, w, cell, dtype=np.int64), np.arange(0, h, cell, dtype=np.int64))
    X1, Y1 = np.minimum(X0 + cell, w) - 1, np.minimum(Y0 + cell, h) - 1
    hit = np.zeros(X0.shape, bool)
    for r in regions:
        x0, y0, x1, y1 = (int(r[k]) for k in ("x0", "y0", "x1", "y1"))
        if int(r["kind"]) == 0:
            hit |= (x0 <= X1) & (x1 >= X0) & (y0 <= Y1) & (y1 >= Y0)
        else:
            dx, dy = x0 - np.clip(x0, X0, X1), y0 - np.clip(y0, Y0, Y1)
            hit |= dx * dx + dy * dy <= x1 * x1
    return int(((X1 - X0 + 1) * (Y1 - Y0 + 1))[hit].sum())


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=1000)
    ap.add_argument("--alt-calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "redact_bench.json"))
    args = ap.parse_args(argv)

    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    rng = np.random.default_rng(3)
    rec = {"method": f"per round: {args.calls} back-to-back hp_redact_* calls on the null stream + one hp_device_synchronize, wall time / calls; then "
                     f"{args.alt_calls} x (hp_memcpy_d2h of the frame into pinned memory + host twin + hp_memcpy_h2d), wall time / calls, and the same "
                     f"for the two copies alone; min and median of {args.rounds} rounds; no profiler, nothing else on the device; pixelate, cell {CELL}, "
                     "margin 1.0; device_gb_per_s = 2 * hit_cell_bytes / median device call (a whole-call rate)",
           "us_per_call": {}}
    rd = frontend.Redactor(2 * max(HUMANS))
    for w, h in SIZES:
        for fmt in FORMATS:
            nbytes = w * h * 3 if fmt == "bgr" else frontend.yuv_packed_bytes(fmt, w, h)
            raw = rng.integers(0, 256, nbytes, dtype=np.uint8)
            if fmt == "p010":
                raw[0::2] &= 0xC0  # a P010 word holds its sample in the high ten bits
            pinned = C.c_void_p()
            _lib.check(L.hp_malloc_host(C.byref(pinned), C.c_size_t(nbytes)))
            for n in HUMANS:
                hs = standing_humans(100 + n, n, w, h)
                for what in WHAT:
                    dev = _lib.DevBuf.from_numpy(raw)  # every configuration starts from the unredacted frame
                    regions = frontend.redact_regions(hs, w, h, what, 1.0)
                    rp, nr = regions.ctypes.data_as(C.c_void_p), len(regions)
                    if fmt == "bgr":
                        def device():
                            return L.hp_redact_u8c3(rd.h, dev.ptr, w, h, w * 3, rp, nr, 0, CELL, None)

                        def host():
                            return L.hp_redact_u8c3_host(pinned, w, h, w * 3, rp, nr, 0, CELL)
                    else:
                        dim, him = image_at(frontend, _lib, fmt, dev.ptr.value, w, h), image_at(frontend, _lib, fmt, pinned.value, w, h)

                        def device():
                            return L.hp_redact_yuv(rd.h, C.byref(dim), rp, nr, 0, CELL, None)

                        def host():
                            return L.hp_redact_yuv_host(C.byref(him), rp, nr, 0, CELL)

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
                    hit_bytes = int(hit_pixels(regions, w, h, CELL) * BYTES_PER_PIXEL[fmt])
                    key = f"{w}x{h} {fmt} {n} humans {what}"
                    rec["us_per_call"][key] = {
                        "regions": int(nr), "frame_bytes": int(nbytes), "hit_cell_bytes": hit_bytes,
                        "device": {"min": round(min(per), 2), "median": round(statistics.median(per), 2)},
                        "device_gb_per_s": round(2 * hit_bytes / statistics.median(per) / 1e3, 1),
                        "d2h_host_h2d": {"min": round(min(alt), 1), "median": round(statistics.median(alt), 1)},
                        "of_which_the_two_copies": {"min": round(min(cp), 1), "median": round(statistics.median(cp), 1)},
                        "ratio_of_medians": round(statistics.median(alt) / statistics.median(per), 1)}
                    print(key, json.dumps(rec["us_per_call"][key]), flush=True)
                    dev.free()
            L.hp_free_host(pinned)
    rd.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
