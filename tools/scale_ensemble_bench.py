"""The scale ensemble measured: what it costs a pipeline, and what its two kernels cost alone.  Alone on the chip, no profiler.

    python tools/scale_ensemble_bench.py [--steps 200] [--rounds 5] [--launches 50000] [--dtypes f32,f16] [--out profiles/scale_ensemble_bench.json]

(a) Pipeline part.  BASELINE configs[1] (Lightweight-OpenPose + PAF parser, 432 x 368), four pipes, device-resident nv12 frames of 1920 x 1080:
frames/s with the ensemble ON (scales 0.5 and 0.75, K = 3) in a pipeline of max_batch 8 K = 24 against OFF in a pipeline of max_batch 8, 8 frames
per submit in both - ON runs 24 network images per batch, OFF 8.  The expectation to confirm or refute is ON ~ OFF / K in frames/s: the network
runs K times per frame (the shrunken passes at full network size: the slot keeps its size, only its content shrinks) and the stage and the merge cost
little beside it.  Method of tools/flip_ensemble_bench.py: clock ramp, then >= `--steps` timed submits with the pipes full, the last result on the
host; the legs alternate round by round in one process.

(b) Kernel part.  LW-OpenPose sizes, n = 4, scales {0.5, 0.75}: hp_scale_stage_u8c3 of 4 slots 432 x 368 into 8, hp_scale_merge of 4 frames over
12 conf maps [19, 46, 54] and over 12 paf maps [38, 46, 54]; `--launches` launches back to back on the null stream + one synchronisation, wall time
per launch, against hipMemcpyAsync device-to-device of the bytes each kernel WRITES, measured the same way in the same rounds.  A launch of this size
lasts about as long as the host needs to issue it: the figures are the cost as a caller pays it, an upper bound of the device time.  (The merge is
timed in place on its own output, launch after launch: the values converge, which changes nothing for a kernel whose time does not depend on the
data.  Its tables are uploaded by the first, untimed call.)
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

FRAME_W, FRAME_H = 1920, 1080
N = 8                 # frames per submit in the pipeline part
SCALES = [0.5, 0.75]  # K = 3
K = len(SCALES) + 1
KN = 4                # the n of the kernel part


def pipeline_part(args) -> dict:
    import bench
    from hyperpose_amd import _lib, frontend
    from hyperpose_amd.engine import Model
    from hyperpose_amd.pipeline import Pipeline
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, (FRAME_H * 3 // 2 // 4, FRAME_W // 4), dtype=np.uint8)
    raw = np.repeat(np.repeat(small, 4, axis=0), 4, axis=1)  # blocky nv12 noise: the parser sees structure, not white noise
    bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, "nv12", FRAME_W, FRAME_H), "nv12")
    images = (_lib.YuvImage * N)(*[frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, FRAME_W, FRAME_H)] * N)
    out = {}
    for dtype in args.dtypes.split(","):
        cfg = bench.config(1, dtype)
        pipes = cfg["pipes"]
        model = Model(cfg["arch"], cfg["w"], cfg["h"])
        weights = model.init_weights(cfg["seed"])
        make = lambda mb: Pipeline(model, weights, max_batch=mb, n_pipes=pipes, keep_ratio=True, max_frame_wh=(cfg["w"], cfg["h"]),  # noqa: E731
                                   parser=cfg["parser"], dtype=cfg["dtype"])
        off, on = make(N), make(K * N)
        on.set_scale_ensemble(SCALES)
        legs = {"off_batch8": off, f"on_batch{K * N}": on}
        fps = {k: [] for k in legs}

        def timed(pl):
            def run(steps):
                for _ in range(steps):
                    if pl.in_flight == pl.n_pipes:
                        pl.collect()
                    pl.submit_yuv_images_raw(images, N, True)

            def drain():
                while pl.in_flight:
                    pl.collect()

            t_ramp = time.perf_counter()
            while time.perf_counter() - t_ramp < 0.3:
                run(2 * pipes)
            drain()
            done, t0 = 0, time.perf_counter()
            while done < args.steps:
                run(2 * pipes)
                done += 2 * pipes
            drain()
            return round(N * done / (time.perf_counter() - t0), 1)

        for _ in range(args.rounds):
            for name, pl in legs.items():
                fps[name].append(timed(pl))
        rec = {name: {"frames_per_submit": N, "frames_per_s_median": statistics.median(v), "frames_per_s_rounds": v} for name, v in fps.items()}
        f_off, f_on = rec["off_batch8"]["frames_per_s_median"], rec[f"on_batch{K * N}"]["frames_per_s_median"]
        rec["on_over_off"] = round(f_on / f_off, 4)
        rec["expected_on_over_off"] = round(1 / K, 4)
        out[dtype] = rec
        print(f"{dtype}: off {f_off} frames/s (max_batch {N}), on {f_on} (K = {K}, max_batch {K * N}); on / off = {rec['on_over_off']} (1 / K = {1 / K:.4f})",
              flush=True)
        for pl in (off, on):
            pl.close()
    return out


def kernel_part(args) -> dict:
    from hyperpose_amd import _lib, frontend
    L = _lib.lib()
    hip = C.CDLL("libamdhip64.so")  # (already in the process: libhp_hip.so links it)
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3  # hipMemcpyDeviceToDevice
    w, h = 432, 368
    mh, mw = 46, 54
    rng = np.random.default_rng(5)
    slot = h * w * 3
    # [4 slots | 8 shrunken slots | room for the copy of those 8]
    frames = _lib.DevBuf.from_numpy(rng.integers(0, 256, ((1 + 2 * (K - 1)) * KN, h, w, 3), dtype=np.uint8))
    stage_bytes = (K - 1) * KN * slot
    cases = {}
    stage = lambda: frontend.scale_stage(frames, frames.ptr.value + KN * slot, w, h, KN, mw, mh, SCALES)  # noqa: E731
    cases[f"scale_stage_u8c3 {KN} x 432x368 -> {(K - 1) * KN}"] = (stage, frames.ptr.value + KN * slot, stage_bytes)
    for name, Cc in ((f"scale_merge conf 19x46x54, K = {K}", 19), (f"scale_merge paf 38x46x54, K = {K}", 38)):
        maps = _lib.DevBuf.from_numpy(rng.standard_normal((K * KN + KN, Cc, mh, mw)).astype(np.float32))
        merge = (lambda maps=maps, Cc=Cc: frontend.scale_merge(maps, KN, K, Cc, mh, mw, SCALES))
        cases[name] = (merge, maps.ptr.value + K * KN * Cc * mh * mw * 4 - KN * Cc * mh * mw * 4, KN * Cc * mh * mw * 4)
    out = {}
    for name, (kernel, src, nbytes) in cases.items():
        def copy(src=src, nbytes=nbytes):  # the bytes the kernel writes, from the last of its inputs into the room behind them
            if hip.hipMemcpyAsync(C.c_void_p(src + nbytes), C.c_void_p(src), nbytes, D2D, None) != 0:
                raise RuntimeError("hipMemcpyAsync failed")

        per = {"kernel": [], "memcpy_d2d": []}
        for _ in range(50):
            kernel(), copy()
        _lib.check(L.hp_device_synchronize())
        for _ in range(args.rounds):
            for which, run in (("kernel", kernel), ("memcpy_d2d", copy)):
                t0 = time.perf_counter()
                for _ in range(args.launches):
                    run()
                _lib.check(L.hp_device_synchronize())
                per[which].append((time.perf_counter() - t0) / args.launches * 1e6)
        rec = {k: {"min": round(min(v), 2), "median": round(statistics.median(v), 2)} for k, v in per.items()}
        rec["bytes_written"] = nbytes
        rec["kernel_over_memcpy"] = round(rec["kernel"]["median"] / rec["memcpy_d2d"]["median"], 3)
        out[name] = rec
        print(f"{name}: kernel {rec['kernel']['median']} us, hipMemcpyAsync D2D of {nbytes} bytes {rec['memcpy_d2d']['median']} us per launch", flush=True)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="timed submits per round of the pipeline part")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50000, help="launches per timed round of the kernel part")
    ap.add_argument("--dtypes", default="f32,f16", help="engine precisions of the pipeline part")
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_ensemble_bench.json"))
    args = ap.parse_args(argv)
    from hyperpose_amd import _lib
    _lib.init(0)
    rec = {"command": f"python tools/scale_ensemble_bench.py --steps {args.steps} --rounds {args.rounds} --launches {args.launches} --dtypes {args.dtypes}"
                      + (" --skip-pipeline" if args.skip_pipeline else ""),
           "scales": SCALES,
           "kernel_method": f"n = {KN}, scales {SCALES}; {args.launches} launches back to back on the null stream + hp_device_synchronize, wall time / "
                            f"launches, min and median of {args.rounds} rounds, kernel and hipMemcpyAsync D2D (of the bytes the kernel writes) alternating; "
                            "no profiler, nothing else on the device",
           "us_per_launch": kernel_part(args)}
    if not args.skip_pipeline:
        rec["pipeline_method"] = (f"BASELINE configs[1], 4 pipes, keep_ratio, device-resident nv12 {FRAME_W}x{FRAME_H}, 0.3 s ramp then >= {args.steps} timed "
                                  f"submits, median of {args.rounds} rounds, legs alternating: off at max_batch {N}, on (K = {K}) at max_batch {K * N}, "
                                  f"{N} frames per submit in both")
        rec["pipeline_frames_per_s"] = pipeline_part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
