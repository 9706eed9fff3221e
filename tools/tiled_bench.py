"""Tiled inference measured: the fused multi-region resize against the same regions as separate launches, and the stream pipeline tiled
against untiled.  Alone on the chip, no profiler.

    python tools/tiled_bench.py [--launches 500] [--rounds 5] [--steps 200] [--out profiles/tiled_bench.json]

Kernel part.  Frames 1920 x 1080 and 3840 x 2160 in device memory as bgr, nv12 and p010; plans of 2 x 2, 3 x 2 and 4 x 3 tiles with 64 px
overlap, letter-boxed into 432 x 368 slots.  `fused`: one hp_resize_rois_* call per frame (ceil(n / 16) launches).  `separate`: n calls of
the per-frame kernel on the same regions - hp_letterbox_u8c3 at pointer offsets, hp_letterbox_yuv on hp_yuv_image descriptions of the
sub-planes.  Per figure: `--launches` frames back to back on the null stream + one synchronisation, wall time per frame, minimum and median
over the rounds; the two forms alternate round by round.  (A launch of this size lasts about as long as the host needs to issue it, so the
`separate` figure is an upper bound of its device time: what the comparison shows is the cost of a frame as a caller pays it.)

Pipeline part.  BASELINE configs[1] (Lightweight-OpenPose + PAF parser, 432 x 368), batch 8, four pipes, keep_ratio, device-resident nv12
frames of 3840 x 2160, fp32 and fp16 engines: frames/s untiled (8 frames per submit) against tiled 2 x 2 / 64 px (R = 4: 2 frames per submit),
by the method of tools/yuv_input_bench.py (clock ramp, then >= `--steps` timed submits, pipes full, the last result on the host).
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

FRAMES = {"1080p": (1920, 1080), "4k": (3840, 2160)}
PLANS = [(2, 2), (3, 2), (4, 3)]
OVERLAP = 64
DW, DH = 432, 368


def _device_frame(fmt, w, h, rng):
    """(source for frontend.resize_rois, description for sub-frames, buffers to keep)"""
    from hyperpose_amd import _lib, frontend
    if fmt == "bgr":
        buf = _lib.DevBuf.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        return buf, None, [buf]
    raw = rng.integers(0, 256, frontend.yuv_packed_bytes(fmt, w, h), dtype=np.uint8)
    bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, fmt, w, h), fmt)
    return frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, w, h), strides, bufs


def _separate_calls(L, fmt, src, strides, w, rois, dst):
    """The per-frame call on every region: [(function, arguments)]"""
    from hyperpose_amd import _lib, frontend
    calls, keep = [], []
    for i, (x, y, rw, rh) in enumerate(rois):
        slot = C.c_void_p(dst.ptr.value + i * DW * DH * 3)
        if fmt == "bgr":
            calls.append((L.hp_letterbox_u8c3, (C.c_void_p(src.ptr.value + (y * w + x) * 3), rw, rh, w * 3, slot, DW, DH, DW * 3, 0, 0, 0, None)))
        else:  # 4:2:0 semi-planar: luma at (x, y), the (U, V) pairs of chroma row y / 2 start at sample x
            sb = _lib.YUV_LAYOUTS[fmt][2]
            sub = frontend.yuv_image(fmt, [src.plane[0] + y * strides[0] + x * sb, src.plane[1] + (y // 2) * strides[1] + x * sb], strides, rw, rh)
            keep.append(sub)
            calls.append((L.hp_letterbox_yuv, (C.byref(sub), slot, DW, DH, DW * 3, 0, 0, 0, None)))
    return calls, keep


def kernel_part(args) -> dict:
    from hyperpose_amd import _lib, frontend
    L = _lib.lib()
    rng = np.random.default_rng(3)
    out = {}
    for fname, (w, h) in FRAMES.items():
        for fmt in ("bgr", "nv12", "p010"):
            src, strides, keep = _device_frame(fmt, w, h, rng)
            for cols, rows in PLANS:
                rois = frontend.plan_tiles(w, h, cols, rows, (OVERLAP, OVERLAP), fmt=None if fmt == "bgr" else fmt)
                dst = _lib.DevBuf(len(rois) * DW * DH * 3)
                calls, keep_sub = _separate_calls(L, fmt, src, strides, w, rois, dst)
                fused = lambda: frontend.resize_rois(src, rois, dst, DW, DH, True, sw=w, sh=h)  # noqa: E731

                def separate():
                    for fn, a in calls:
                        fn(*a)

                per = {"fused": [], "separate": []}
                for _ in range(50):
                    fused(), separate()
                _lib.check(L.hp_device_synchronize())
                for _ in range(args.rounds):
                    for name, run in (("fused", fused), ("separate", separate)):
                        t0 = time.perf_counter()
                        for _ in range(args.launches):
                            run()
                        _lib.check(L.hp_device_synchronize())
                        per[name].append((time.perf_counter() - t0) / args.launches * 1e6)
                rec = {k: {"min": round(min(v), 2), "median": round(statistics.median(v), 2)} for k, v in per.items()}
                rec["regions"] = len(rois)
                rec["fused_over_separate"] = round(rec["fused"]["median"] / rec["separate"]["median"], 3)
                out[f"{fname} {fmt} {cols}x{rows}"] = rec
                print(f"{fname} {fmt} {cols}x{rows}: fused {rec['fused']['median']} us, separate {rec['separate']['median']} us per frame", flush=True)
                del keep_sub
            del keep
    return out


def pipeline_part(args) -> dict:
    import bench
    from hyperpose_amd import _lib, frontend
    from hyperpose_amd.engine import Model
    from hyperpose_amd.pipeline import Pipeline
    w, h = FRAMES["4k"]
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, (h // 8 * 3 // 2, w // 8), dtype=np.uint8)
    raw = np.repeat(np.repeat(small, 8, axis=0), 8, axis=1)  # blocky nv12 noise: the parser sees structure, not white noise
    bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, "nv12", w, h), "nv12")
    out = {}
    for dtype in ("f32", "f16"):
        cfg = bench.config(1, dtype)
        batch, pipes = cfg["batch"], cfg["pipes"]
        model = Model(cfg["arch"], cfg["w"], cfg["h"])
        # (device frames: nothing is staged, so the staging buffers need not hold a 4K frame)
        pl = Pipeline(model, model.init_weights(cfg["seed"]), max_batch=batch, n_pipes=pipes, keep_ratio=True, max_frame_wh=(cfg["w"], cfg["h"]),
                      parser=cfg["parser"], dtype=cfg["dtype"])
        images = (_lib.YuvImage * batch)(*[frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, w, h)] * batch)
        rec = {}
        for name, tiles in (("untiled", None), ("tiled 2x2", (2, 2))):
            pl.set_tiling(*tiles, overlap=(OVERLAP, OVERLAP)) if tiles else pl.set_tiling(None)
            n = batch // (tiles[0] * tiles[1]) if tiles else batch

            def run(steps):
                for _ in range(steps):
                    if pl.in_flight == pl.n_pipes:
                        pl.collect()
                    pl.submit_yuv_images_raw(images, n, True)

            def drain():
                while pl.in_flight:
                    pl.collect()

            fps = []
            for _ in range(args.rounds):
                t_ramp = time.perf_counter()
                while time.perf_counter() - t_ramp < 0.3:
                    run(2 * pipes)
                drain()
                done, t0 = 0, time.perf_counter()
                while done < args.steps:
                    run(2 * pipes)
                    done += 2 * pipes
                drain()
                fps.append(round(n * done / (time.perf_counter() - t0), 1))
            rec[name] = {"frames_per_submit": n, "frames_per_s_median": statistics.median(fps), "frames_per_s_rounds": fps}
            print(f"{dtype} {name}: {statistics.median(fps)} frames/s", flush=True)
        rec["tiled_over_untiled"] = round(rec["tiled 2x2"]["frames_per_s_median"] / rec["untiled"]["frames_per_s_median"], 4)
        out[dtype] = rec
        pl.close()
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=500, help="frames per timed round of the kernel part")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200, help="timed submits per round of the pipeline part")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiled_bench.json"))
    args = ap.parse_args(argv)
    from hyperpose_amd import _lib
    _lib.init(0)
    # the command line with every measurement parameter spelled out (where the record is written does not belong to the measurement)
    rec = {"command": f"python tools/tiled_bench.py --launches {args.launches} --rounds {args.rounds} --steps {args.steps}" + (" --skip-pipeline" if args.skip_pipeline else ""),
           "kernel_method": f"{args.launches} frames back to back on the null stream + hp_device_synchronize, wall time / frames, min and median of {args.rounds} "
                            f"rounds, fused and separate alternating; {OVERLAP} px overlap, letter-boxed into {DW}x{DH} slots; no profiler, nothing else on the device",
           "us_per_frame": kernel_part(args)}
    if not args.skip_pipeline:
        rec["pipeline_method"] = (f"BASELINE configs[1], batch 8, 4 pipes, keep_ratio, device-resident nv12 3840x2160, 0.3 s ramp then >= {args.steps} timed submits, "
                                  f"median of {args.rounds} rounds; tiled: 2x2 tiles, {OVERLAP} px overlap, 2 frames per submit")
        rec["pipeline_frames_per_s"] = pipeline_part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
