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

`--formats` selects the feeds (default `bgr,nv12`, the record above).  Beside those two: `nv12-image`, `p010`, `yuy2` (and any other layout
name) go through hp_pipeline_submit_yuv_images from pinned host memory - P010 moves 3 bytes per pixel like BGR, YUY2 2, NV12 1.5 - and
`<layout>-device` submits the same frames as device-resident surfaces uploaded before the timed region (no H2D copy at all).  The record
of all of them is profiles/yuv_formats_bench.json:

    python tools/yuv_input_bench.py --formats bgr,nv12,nv12-image,p010,yuy2,nv12-device,p010-device,p010-hdr,p010-hdr-device --out profiles/yuv_formats_bench.json

`<layout>-hdr` and `<layout>-hdr-device` (10-bit layouts) are the very bytes of `<layout>` / `<layout>-device` on a pipeline with
Pipeline.set_tonemap("pq"): the frames go through resize_yuv_hdr_kernel instead of resize_yuv_word16_kernel.  Each HDR feed is reported against its
SDR twin: the ratio of the medians, the difference in frames/s and whether it lies within the larger of the two feeds' own spreads.
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

    def __init__(self, model, weights, cfg, frames: np.ndarray, fmt: str, layout: str = None, on_device: bool = False, hdr: bool = False):
        """`frames`: [batch, bytes...] uint8, one tightly packed frame per row.  `fmt` "bgr" / "nv12" are the two legacy calls; with `layout`
        the frames go through hp_pipeline_submit_yuv_images (BT.601 limited), from pinned host memory or, `on_device`, from device memory."""
        from hyperpose_amd import _lib, frontend
        from hyperpose_amd.pipeline import Pipeline
        self.fmt, self.batch = fmt, frames.shape[0]
        self.nbytes = frames[0].nbytes
        self.h2d_bytes = 0 if on_device else self.nbytes
        self._lib = _lib.lib()
        self.host = C.c_void_p()
        _lib.check(self._lib.hp_malloc_host(C.byref(self.host), C.c_size_t(frames.nbytes)))
        src = np.ascontiguousarray(frames)
        C.memmove(self.host, src.ctypes.data, src.nbytes)
        b = self.batch
        self.ptrs = (C.POINTER(C.c_uint8) * b)(*[C.cast(self.host.value + i * self.nbytes, C.POINTER(C.c_uint8)) for i in range(b)])
        self.ws, self.hs = (C.c_int * b)(*([FRAME_W] * b)), (C.c_int * b)(*([FRAME_H] * b))
        self.images, self.on_device, self.dev = None, on_device, None
        if layout:
            base = self.host.value
            if on_device:  # the surfaces are uploaded (and complete: hp_memcpy_h2d is synchronous) before anything is timed
                self.dev = _lib.DevBuf.from_numpy(src)
                base = self.dev.ptr.value
            self.images = (_lib.YuvImage * b)()
            for i in range(b):
                at, planes, strides = base + i * self.nbytes, [], []
                for rows, cols in frontend.yuv_plane_shapes(layout, FRAME_W, FRAME_H):
                    row = cols * _lib.YUV_LAYOUTS[layout][2]
                    planes.append(at), strides.append(row)
                    at += rows * row
                self.images[i] = frontend.yuv_image(layout, planes, strides, FRAME_W, FRAME_H)
        self.pl = Pipeline(model, weights, max_batch=b, n_pipes=cfg["pipes"], keep_ratio=True, max_frame_wh=(FRAME_W, FRAME_H), parser=cfg["parser"],
                           dtype=cfg["dtype"])
        if hdr:
            self.pl.set_tonemap("pq")
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
            if self.images is not None:
                pl.submit_yuv_images_raw(self.images, self.batch, self.on_device)
            elif self.fmt == "bgr":
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
        if self.dev is not None:
            self.dev.free()


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
                for key in ("resize_u8c3_kernel", "resize_yuv420_kernel", "resize_yuv_planar8_kernel", "resize_yuv_packed8_kernel", "resize_yuv_word16_kernel",
                            "resize_yuv_hdr_kernel"):
                    if key in name:
                        out[key] = {"calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                                    "min_us": round(float(row["MinNs"]) / 1e3, 2), "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400, help="timed steps per round and path (rounded up to whole chunks of 2 x pipes)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_input_bench.json"))
    ap.add_argument("--formats", default="bgr,nv12", help="comma-separated feeds: bgr, nv12 (the two legacy calls), <layout> or nv12-image (hp_pipeline_submit_yuv_images "
                                                         "from pinned host memory), <layout>-device (device-resident surfaces)")
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
    big = np.repeat(np.repeat(small, 8, axis=1), 8, axis=2)
    nv12 = synth.bgr_to_yuv420(big, "nv12")
    bgr = np.stack([nv12_to_bgr(f) for f in nv12])

    names = [n.strip() for n in args.formats.split(",") if n.strip()]
    feeds, kernels = {}, {}
    for name in names:
        if name == "bgr":
            feeds[name], kernels[name] = Feed(model, weights, cfg, bgr, "bgr"), "resize_u8c3_kernel"
        elif name == "nv12":
            feeds[name], kernels[name] = Feed(model, weights, cfg, nv12, "nv12"), "resize_yuv420_kernel"
        else:
            layout = name.split("-")[0]
            hdr = "hdr" in name.split("-")[1:]
            if layout not in _lib.YUV_LAYOUTS or name.split("-")[1:] not in ([], ["image"], ["device"], ["hdr"], ["hdr", "device"]) or (
                    hdr and _lib.YUV_LAYOUTS[layout][2] != 2):
                ap.error(f"--formats: {name!r} is not bgr, nv12, <layout>, <layout>-image, <layout>-device or, for a 10-bit layout, <layout>-hdr[-device]")
            # NV12 feeds carry the legacy feed's very bytes (same humans); the other layouts the same pictures through the input generator
            packed = nv12.reshape(batch, -1) if layout == "nv12" else np.stack(
                [np.concatenate([p.view(np.uint8).ravel() for p in f]) for f in synth.bgr_to_yuv(big, layout)])
            feeds[name] = Feed(model, weights, cfg, packed, name, layout=layout, on_device=name.endswith("-device"), hdr=hdr)
            kernels[name] = "resize_yuv_hdr_kernel" if hdr else {1: "resize_yuv_packed8_kernel"}.get(_lib.YUV_LAYOUTS[layout][1], "resize_yuv_word16_kernel" if _lib.YUV_LAYOUTS[layout][2] == 2
                                                               else "resize_yuv_planar8_kernel")
    chunk = max(2 * cfg["pipes"], 4)
    rounds = {name: [] for name in names}
    for r in range(args.rounds):
        for name in names:
            fps = feeds[name].timed(args.steps, chunk)
            rounds[name].append(round(fps, 1))
            print(f"round {r} {name}: {fps:.1f} frames/s", flush=True)
    # every feed that carries the NV12 bytes (or their host conversion) must return the same humans
    same_set = [n for n in names if n == "bgr" or n.split("-")[0] == "nv12"]
    same = all(a.tobytes() == b.tobytes() for n in same_set[1:] for a, b in zip(feeds[same_set[0]].first, feeds[n].first))
    rec = {"workload": f"{cfg['label']}, data_type::kFLOAT, batch {batch}, {cfg['pipes']} pipes, keep_ratio, {FRAME_W}x{FRAME_H} frames in pinned host memory, "
                       f">= {args.steps} timed steps per round, {' and '.join(n.upper() if n in ('bgr', 'nv12') else n for n in names)} rounds alternating in one process",
           "same_humans_first_batch": bool(same)}
    if names != ["bgr", "nv12"]:
        rec["same_humans_compared"] = same_set
    for name in names:
        v = rounds[name]
        rec[name] = {"frames_per_s_median": statistics.median(v), "frames_per_s_rounds": v, "spread": round(max(v) - min(v), 1),
                     "h2d_bytes_per_frame": int(feeds[name].h2d_bytes), "kernel": kernels[name]}
    margin = max(rec[n]["spread"] for n in names)
    for name in names:
        for base in ("bgr", "nv12"):
            if base in names and name != base and (name, base) != ("bgr", "nv12"):
                rec[f"{name}_over_{base}"] = round(rec[name]["frames_per_s_median"] / rec[base]["frames_per_s_median"], 4)
                key = "nv12_not_slower_within_spread" if (name, base) == ("nv12", "bgr") else f"{name}_not_slower_than_{base}_within_spread"
                rec[key] = bool(rec[name]["frames_per_s_median"] >= rec[base]["frames_per_s_median"] - margin)
    for name in names:  # every HDR feed against its SDR twin
        twin = name.replace("-hdr", "")
        if twin != name and twin in names:
            a, b = rec[name], rec[twin]
            yard = max(a["spread"], b["spread"])
            rec[f"{name}_over_{twin}"] = round(a["frames_per_s_median"] / b["frames_per_s_median"], 4)
            rec[f"{name}_minus_{twin}_frames_per_s"] = round(a["frames_per_s_median"] - b["frames_per_s_median"], 1)
            rec[f"{name}_within_larger_spread_of_{twin}"] = bool(abs(a["frames_per_s_median"] - b["frames_per_s_median"]) <= yard)
    for f in feeds.values():
        f.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
