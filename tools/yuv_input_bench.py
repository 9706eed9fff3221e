"""NV12 input against BGR input through the stream pipeline, in ONE process (modelled on bench.py's `from_host`, which stays as it is).

    python tools/yuv_input_bench.py [--steps 400] [--rounds 3] [--out profiles/yuv_input_bench.json]

Workload: BASELINE configs[1] (Lightweight-OpenPose + PAF parser, 432 x 368) at data_type::kFLOAT, batch 8, four pipes, keep_ratio, 1280 x 720
frames in pinned host memory.  The same pictures are submitted as 8-bit BGR (hp_pipeline_submit: 2.76 MB per frame over PCIe, resize_u8c3_kernel)
and as NV12 (hp_pipeline_submit_yuv: 1.38 MB per frame, resize_yuv420_kernel).  The two paths alternate round by round - BGR, NV12, BGR, NV12, ... -
on two pipelines that live side by side, each round >= `--steps` timed steps after a clock ramp, pipes full throughout; the figure of a path
is the median of its rounds and the spread (max - min over its rounds) is reported with it: that spread is the yardstick for "not slower".

Kernel times come from a separate run of this tool under the profiler:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/yuv_input_bench.py --steps 40 --rounds 1 --out <dir>/bench.json

and are merged into the JSON with `--kernel-stats <dir>` (reads the *kernel_stats.csv the profiler wrote).
"""
from __future__ import annotations

import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAME_W, FRAME_H = 1280, 720


class Feed:
    """One pipeline fed from pinned host memory with pre-marshalled pointers, as bench.py's HostFed does."""

    def __init__(self, model, weights, cfg, frames: np.ndarray, fmt: str):
        from hyperpose_amd import _lib
        from hyperpose_amd.pipeline import Pipeline
        self.fmt, self.batch = fmt, frames.shape[0]
        self.nbytes = frames[0].nbytes
        self._lib = _lib.lib()
        self.host = C.c_void_p()
        _lib.check(self._lib.hp_malloc_host(C.byref(self.host), C.c_size_t(frames.nbytes)))
        src = np.ascontiguousarray(frames)
        C.memmove(self.host, src.ctypes.data, src.nbytes)
        b = self.batch
        self.ptrs = (C.POINTER(C.c_uint8) * b)(*[C.cast(self.host.value + i * self.nbytes, C.POINTER(C.c_uint8)) for i in range(b)])
        self.ws, self.hs = (C.c_int * b)(*([FRAME_W] * b)), (C.c_int * b)(*([FRAME_H] * b))
        self.pl = Pipeline(model, weights, max_batch=b, n_pipes=cfg["pipes"], keep_ratio=True, max_frame_wh=(FRAME_W, FRAME_H), parser=cfg["parser"],
                           dtype=cfg["dtype"])
        self.humans = 0
        self.first = None  # the humans of the first batch collected (the two feeds are compared on it)

    def _collect(self):
        got = self.pl.collect()
        if self.first is None:
            self.first = got
        self.humans += sum(len(h) for h in got)

    def run(self, n: int):
        pl = self.pl
        for _ in range(n):
            if pl.in_flight == pl.n_pipes:
                self._collect()
            if self.fmt == "bgr":
                pl.submit_ptrs(self.ptrs, self.ws, self.hs, self.batch)
            else:
                pl.submit_yuv_ptrs(self.fmt, self.ptrs, self.ws, self.hs, self.batch)

    def drain(self):
        while self.pl.in_flight:
            self._collect()

    def timed(self, steps: int, chunk: int) -> float:
        """frames/s over >= `steps` steps: 0.3 s clock ramp (untimed, drained), then whole chunks; the timed region starts with empty pipes and
        ends when the last result is on the host"""
        t_ramp = time.perf_counter()
        while time.perf_counter() - t_ramp < 0.3:
            self.run(chunk)
        self.drain()
        done = 0
        t0 = time.perf_counter()
        while done < steps:
            self.run(chunk)
            done += chunk
        self.drain()
        return self.batch * done / (time.perf_counter() - t0)

    def close(self):
        self.drain()
        self.pl.close()
        self._lib.hp_free_host(self.host)


def nv12_to_bgr(frame: np.ndarray) -> np.ndarray:
    """cv::cvtColor(COLOR_YUV2BGR_NV12) on the host (the fixed-point BT.601 form hp_resize_yuv420 evaluates), so that the BGR feed carries
    the very pictures the NV12 feed does and the two must return the same humans."""
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    y = frame[:h].astype(np.int32)
    uv = frame[h:].reshape(h // 2, w // 2, 2).astype(np.int32) - 128
    u, v = (np.repeat(np.repeat(uv[..., c], 2, axis=0), 2, axis=1) for c in range(2))
    yy = np.maximum(0, y - 16) * 1220542 + (1 << 19)
    out = np.stack([(yy + 2116026 * u) >> 20, (yy - 852492 * v - 409993 * u) >> 20, (yy + 1673527 * v) >> 20], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def kernel_times(stats_dir: str) -> dict:
    """Average duration (us) and call count of the two front-end kernels from rocprofv3's kernel_stats.csv under `stats_dir`."""
    out = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key in ("resize_u8c3_kernel", "resize_yuv420_kernel"):
                    if key in name:
                        out[key] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                    "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400, help="timed steps per round and path (rounded up to whole chunks of 2 x pipes)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_input_bench.json"))
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge the kernel times into --out and exit")
    args = ap.parse_args(argv)

    if args.kernel_stats:
        rec = json.load(open(args.out)) if os.path.exists(args.out) else {}
        rec["kernel_time"] = kernel_times(args.kernel_stats)
        rec["kernel_time"]["source"] = ("one rocprofv3 --kernel-trace --stats run of this tool (--steps 40 --rounds 1); one launch = one 1280x720 frame "
                                        "letter-boxed into 432x368")
        json.dump(rec, open(args.out, "w"), indent=1)
        print(json.dumps(rec["kernel_time"]))
        return 0

    import bench
    from hyperpose_amd import _lib, synth
    from hyperpose_amd.engine import Model
    _lib.init(0)
    cfg = bench.config(1, "f32")
    batch = cfg["batch"]
    model = Model(cfg["arch"], cfg["w"], cfg["h"])
    weights = model.init_weights(cfg["seed"])
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, (batch, FRAME_H // 8, FRAME_W // 8, 3), dtype=np.uint8)
    nv12 = synth.bgr_to_yuv420(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2), "nv12")
    bgr = np.stack([nv12_to_bgr(f) for f in nv12])

    feeds = {"bgr": Feed(model, weights, cfg, bgr, "bgr"), "nv12": Feed(model, weights, cfg, nv12, "nv12")}
    chunk = max(2 * cfg["pipes"], 4)
    rounds = {"bgr": [], "nv12": []}
    for r in range(args.rounds):
        for name in ("bgr", "nv12"):
            fps = feeds[name].timed(args.steps, chunk)
            rounds[name].append(round(fps, 1))
            print(f"round {r} {name}: {fps:.1f} frames/s", flush=True)
    same = all(a.tobytes() == b.tobytes() for a, b in zip(feeds["bgr"].first, feeds["nv12"].first))
    rec = {"workload": f"{cfg['label']}, data_type::kFLOAT, batch {batch}, {cfg['pipes']} pipes, keep_ratio, {FRAME_W}x{FRAME_H} frames in pinned host memory, "
                       f">= {args.steps} timed steps per round, BGR and NV12 rounds alternating in one process",
           "same_humans_first_batch": bool(same)}
    for name in ("bgr", "nv12"):
        v = rounds[name]
        rec[name] = {"frames_per_s_median": statistics.median(v), "frames_per_s_rounds": v, "spread": round(max(v) - min(v), 1),
                     "h2d_bytes_per_frame": int(feeds[name].nbytes), "kernel": "resize_u8c3_kernel" if name == "bgr" else "resize_yuv420_kernel"}
    margin = max(rec["bgr"]["spread"], rec["nv12"]["spread"])
    rec["nv12_over_bgr"] = round(rec["nv12"]["frames_per_s_median"] / rec["bgr"]["frames_per_s_median"], 4)
    rec["nv12_not_slower_within_spread"] = bool(rec["nv12"]["frames_per_s_median"] >= rec["bgr"]["frames_per_s_median"] - margin)
    for f in feeds.values():
        f.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
