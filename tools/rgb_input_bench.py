"""Packed RGB / BGRA / grey input (hp_rgb_image) against what a caller had to do before it existed, on the MI355X.

    python tools/rgb_input_bench.py [--launches 2000] [--rounds 3] [--steps 200] [--out profiles/rgb_input_bench.json]

(a) Kernels alone, us per launch: back-to-back launches on the null stream + one synchronisation, wall time / launches (tools/yuv_kernel_bench.py's
method; no profiler, nothing else on the device).  Every layout through hp_resize_rgb beside hp_resize_oriented_u8c3 on a BGR24 frame of the same
size, 1280 x 720 and 1920 x 1080 letter-boxed into the Lightweight-OpenPose input (432 x 368) - launches so short that the host's issue time shows, not
the kernel's - and 1280 x 720 -> 2560 x 1440, where the device time dominates; orientation code 0 and a quarter turn (code 1).  The
thread map (HP_ORIENT_MAP=rows|cols) and the Taps type of the 4-byte layouts (HP_RGB_TAPS=bytes|words) are read once per process, so every
(map, taps) pair is a child process of this tool; the children alternate round by round and never overlap.  Per figure: the median over the rounds
and the spread (max - min).  `words_over_bytes` is the ratio of the medians of the 4-byte layouts, one 32-bit load per tap against three byte loads.

(b) The stream, frames/s and H2D bytes per frame: BASELINE configs[1] at data_type::kFLOAT (tools/yuv_input_bench.py's workload: batch 8, four
pipes, keep_ratio, frames in pinned host memory, pipes full, rounds alternating in ONE process on ONE pipeline).  Feeds:
    bgra, gray           hp_pipeline_submit_rgb_images from pinned host memory
    bgra-device          the same BGRA frames as device-resident surfaces (no copy)
    bgra-repack, gray-repack   what a caller does today: every frame repacked to BGR24 on the host (hp_rgb_to_bgr_host, one thread, into pinned
                         memory) INSIDE the timed loop, then hp_pipeline_submit
All feeds of one size carry the same pictures and must return the same humans (grey feeds among themselves).
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [(1280, 720), (1920, 1080)]
NET_W, NET_H = 432, 368
# (name, sw, sh, dw, dh, keep_ratio): the stream's own two, where a launch lasts about as long as the host needs to issue it, and - as in
# tools/yuv_kernel_bench.py - one with 23 times the output pixels, where the device time dominates and the Taps can be told apart
GEOMETRIES = [("1280x720", 1280, 720, NET_W, NET_H, 1), ("1920x1080", 1920, 1080, NET_W, NET_H, 1), ("1280x720->2560x1440", 1280, 720, 2560, 1440, 0)]
CODES = [0, 1]


def stat(v):
    return {"median": round(statistics.median(v), 2), "spread": round(max(v) - min(v), 2), "rounds": [round(x, 2) for x in v]}


# ---- (a) one child: every feed under the (map, taps) of its environment --------------------------------------------------------------------

def kernel_child(launches: int) -> int:
    from hyperpose_amd import _lib, frontend
    _lib.init(0)
    L = _lib.lib()
    rng = np.random.default_rng(3)
    dst = _lib.DevBuf(2560 * 1440 * 3)
    out = {}
    for gname, sw, sh, dw, dh, keep_ratio in GEOMETRIES:
        calls, keep = {}, []
        for code in CODES:
            bgr = _lib.DevBuf.from_numpy(rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8))
            keep.append(bgr)
            calls[f"u8c3 code {code}"] = (L.hp_resize_oriented_u8c3, (bgr.ptr, sw, sh, sw * 3, code, keep_ratio, 0, 0, 0, dst.ptr, dw, dh, dw * 3, None))
            for fmt, (_, pb, *_r) in _lib.RGB_LAYOUTS.items():
                src = _lib.DevBuf.from_numpy(rng.integers(0, 256, sh * sw * pb, dtype=np.uint8))
                im = frontend.rgb_image(fmt, src, sw, sh)
                keep += [src, im]
                calls[f"{fmt} code {code}"] = (L.hp_resize_rgb, (C.byref(im), code, keep_ratio, 0, 0, 0, dst.ptr, dw, dh, dw * 3, None))
        for name, (fn, a) in calls.items():
            for _ in range(200):
                _lib.check(fn(*a))
            _lib.check(L.hp_device_synchronize())
            t0 = time.perf_counter()
            for _ in range(launches):
                fn(*a)
            _lib.check(L.hp_device_synchronize())
            out[f"{gname} {name}"] = (time.perf_counter() - t0) / launches * 1e6
        del keep
    print("KERNELS " + json.dumps(out), flush=True)
    return 0


def kernels(args) -> dict:
    combos = [(m, t) for m in ("rows", "cols") for t in ("bytes", "words")]
    raw = {c: {} for c in combos}
    for r in range(args.rounds):
        for m, t in combos:
            env = dict(os.environ, HP_ORIENT_MAP=m, HP_RGB_TAPS=t)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-child", "--launches", str(args.launches)], env=env, capture_output=True,
                               text=True, timeout=300)
            line = [ln for ln in p.stdout.splitlines() if ln.startswith("KERNELS ")]
            if p.returncode != 0 or not line:
                raise RuntimeError(f"kernel child {m} {t} failed ({p.returncode}): {p.stdout[-1000:]}{p.stderr[-2000:]}")
            for k, v in json.loads(line[0][8:]).items():
                raw[m, t].setdefault(k, []).append(v)
            print(f"round {r} map {m} taps {t}: done", flush=True)
    rec = {"method": f"{args.launches} back-to-back launches on the null stream + hp_device_synchronize, wall time / launches; one child process per "
                     f"(thread map, taps) pair, {args.rounds} rounds alternating; median and spread (max - min) over the rounds; "
                     f"1280x720 and 1920x1080 are letter-boxed into {NET_W}x{NET_H} (launch-bound), 1280x720->2560x1440 is device-bound",
           "us_per_launch": {}, "words_over_bytes": {}, "layout_over_u8c3": {}}
    for (m, t), feeds in raw.items():
        rec["us_per_launch"][f"map {m}, taps {t}"] = {k: stat(v) for k, v in feeds.items()}
    for m in ("rows", "cols"):
        b, w = rec["us_per_launch"][f"map {m}, taps bytes"], rec["us_per_launch"][f"map {m}, taps words"]
        rec["words_over_bytes"][f"map {m}"] = {k: {"ratio": round(w[k]["median"] / b[k]["median"], 3),
                                                   "wins_by_more_than_spread": bool(b[k]["median"] - w[k]["median"] > max(b[k]["spread"], w[k]["spread"]))}
                                               for k in b if any(f" {f} " in k for f in ("bgra", "rgba", "argb", "abgr"))}
    # each layout beside the BGR kernel under the map the library picks for the code (rows for code 0, cols for the quarter turn) and the default taps
    for code, m in ((0, "rows"), (1, "cols")):
        d = rec["us_per_launch"][f"map {m}, taps words"]
        for k in d:
            if k.endswith(f"code {code}") and " u8c3 " not in k:
                base = d[k.split(" ")[0] + f" u8c3 code {code}"]
                rec["layout_over_u8c3"][k] = {"us": d[k]["median"], "u8c3_us": base["median"], "ratio": round(d[k]["median"] / base["median"], 3)}
    return rec


# ---- (b) the stream -------------------------------------------------------------------------------------------------------------------------

class Feed:
    def __init__(self, pl, kind: str, frames: np.ndarray, fmt: str, w: int, h: int):
        """`frames`: [batch, ...] uint8 frames of layout `fmt`; kind "host" | "device" | "repack"."""
        from hyperpose_amd import _lib, frontend
        self.pl, self.kind, self.batch, self.L = pl, kind, frames.shape[0], _lib.lib()
        b, self.nbytes = self.batch, frames[0].nbytes
        self.host = C.c_void_p()
        _lib.check(self.L.hp_malloc_host(C.byref(self.host), C.c_size_t(frames.nbytes)))
        C.memmove(self.host, np.ascontiguousarray(frames).ctypes.data, frames.nbytes)
        base, self.dev, self.bgr = self.host.value, None, None
        if kind == "device":
            self.dev = _lib.DevBuf.from_numpy(frames)
            base = self.dev.ptr.value
        self.images = (_lib.RgbImage * b)(*[frontend.rgb_image(fmt, base + i * self.nbytes, w, h) for i in range(b)])
        self.h2d_bytes = 0 if kind == "device" else self.nbytes
        if kind == "repack":  # one pinned BGR24 buffer per batch in flight (+ the one being filled), as a caller would keep
            self.ring, self.at = [], 0
            for _ in range(pl.n_pipes + 1):
                p = C.c_void_p()
                _lib.check(self.L.hp_malloc_host(C.byref(p), C.c_size_t(b * w * h * 3)))
                ptrs = (C.POINTER(C.c_uint8) * b)(*[C.cast(p.value + i * w * h * 3, C.POINTER(C.c_uint8)) for i in range(b)])
                self.ring.append((p, ptrs))
            self.ws, self.hs, self.w, self.h = (C.c_int * b)(*([w] * b)), (C.c_int * b)(*([h] * b)), w, h
            self.h2d_bytes = w * h * 3
        self.first = None

    def _collect(self):
        got = self.pl.collect()
        if self.first is None:
            self.first = got

    def run(self, n: int):
        pl = self.pl
        for _ in range(n):
            if pl.in_flight == pl.n_pipes:
                self._collect()
            if self.kind == "repack":
                p, ptrs = self.ring[self.at]
                self.at = (self.at + 1) % len(self.ring)
                for i in range(self.batch):
                    self.L.hp_rgb_to_bgr_host(C.byref(self.images[i]), C.c_void_p(p.value + i * self.w * self.h * 3), self.w * 3)
                pl.submit_ptrs(ptrs, self.ws, self.hs, self.batch)
            else:
                pl.submit_rgb_images_raw(self.images, self.batch, self.kind == "device")

    def drain(self):
        while self.pl.in_flight:
            self._collect()

    def timed(self, steps: int, chunk: int) -> float:
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < 0.3:
            self.run(chunk)
        self.drain()
        done, t0 = 0, time.perf_counter()
        while done < steps:
            self.run(chunk)
            done += chunk
        self.drain()
        return self.batch * done / (time.perf_counter() - t0)

    def close(self):
        self.drain()
        self.L.hp_free_host(self.host)
        for p, _ in getattr(self, "ring", []):
            self.L.hp_free_host(p)
        if self.dev is not None:
            self.dev.free()


def stream(args) -> dict:
    import bench
    from hyperpose_amd import _lib
    from hyperpose_amd.engine import Model
    from hyperpose_amd.pipeline import Pipeline
    _lib.init(0)
    cfg = bench.config(1, "f32")
    batch = cfg["batch"]
    model = Model(cfg["arch"], cfg["w"], cfg["h"])
    pl = Pipeline(model, model.init_weights(cfg["seed"]), max_batch=batch, n_pipes=cfg["pipes"], keep_ratio=True, max_frame_wh=(1920, 1440),
                  parser=cfg["parser"], dtype=cfg["dtype"])
    rec = {"workload": f"{cfg['label']}, data_type::kFLOAT, batch {batch}, {cfg['pipes']} pipes, keep_ratio, frames in pinned host memory, >= {args.steps} timed "
                       f"steps per round, {args.rounds} rounds alternating in one process on one pipeline; repack = hp_rgb_to_bgr_host per frame, one thread, "
                       "inside the timed loop", "sizes": {}}
    chunk = max(2 * cfg["pipes"], 4)
    rng = np.random.default_rng(7)
    ok = True
    for w, h in SIZES:
        small = rng.integers(0, 256, (batch, h // 8, w // 8, 4), dtype=np.uint8)
        bgra = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))
        gray = np.ascontiguousarray(bgra[..., 1])
        feeds = {"bgra-repack": Feed(pl, "repack", bgra, "bgra", w, h), "bgra": Feed(pl, "host", bgra, "bgra", w, h),
                 "bgra-device": Feed(pl, "device", bgra, "bgra", w, h), "gray-repack": Feed(pl, "repack", gray, "gray", w, h),
                 "gray": Feed(pl, "host", gray, "gray", w, h)}
        rounds = {k: [] for k in feeds}
        for r in range(args.rounds):
            for k, f in feeds.items():
                rounds[k].append(f.timed(args.steps, chunk))
                print(f"{w}x{h} round {r} {k}: {rounds[k][-1]:.1f} frames/s", flush=True)
        same = all(a.tobytes() == b.tobytes() for base, others in (("bgra-repack", ("bgra", "bgra-device")), ("gray-repack", ("gray",)))
                   for o in others for a, b in zip(feeds[base].first, feeds[o].first))
        ok = ok and same
        out = {"same_humans_first_batch": bool(same)}
        for k, v in rounds.items():
            out[k] = {"frames_per_s": stat(v), "h2d_bytes_per_frame": int(feeds[k].h2d_bytes)}
        for k, base in (("bgra", "bgra-repack"), ("bgra-device", "bgra-repack"), ("gray", "gray-repack")):
            a, b = out[k]["frames_per_s"], out[base]["frames_per_s"]
            out[f"{k}_over_{base}"] = {"ratio": round(a["median"] / b["median"], 3),
                                       "wins_by_more_than_spread": bool(a["median"] - b["median"] > max(a["spread"], b["spread"]))}
        rec["sizes"][f"{w}x{h}"] = out
        for f in feeds.values():
            f.close()
    pl.close()
    rec["ok"] = bool(ok)
    return rec


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--part", default="kernels,stream")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rgb_input_bench.json"))
    ap.add_argument("--kernel-child", action="store_true", help="internal: one (map, taps) measurement, printed as one line")
    args = ap.parse_args(argv)
    if args.kernel_child:
        return kernel_child(args.launches)
    rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if "kernels" in args.part:  # before this process opens the device: the children have it to themselves
        rec["kernels"] = kernels(args)
    if "stream" in args.part:
        rec["stream"] = stream(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if rec.get("stream", {}).get("ok", True) else 1


if __name__ == "__main__":
    sys.exit(main())
