"""The flip ensemble measured: what it costs a pipeline, and what its two kernels cost alone.  Alone on the chip, no profiler.

    python tools/flip_ensemble_bench.py [--steps 200] [--rounds 5] [--launches 50000] [--out profiles/flip_ensemble_bench.json]

(a) Pipeline part.  BASELINE configs[1] (Lightweight-OpenPose + PAF parser, 432 x 368), four pipes, device-resident nv12 frames of 1920 x 1080, fp32
(kFLOAT) and fp16 (kHALF) engines: frames/s with the ensemble ON in a pipeline of max_batch 16 against OFF in a pipeline of max_batch 8, 8 frames
per submit in both - ON runs 16 network images per batch, OFF 8 - and the expectation to confirm or refute is ON ~ OFF / 2 in frames/s: the
network runs twice per frame and the flip, the copy of the originals and the merge cost little beside it.  A third leg runs the 16-image pipeline with the
ensemble off on 16 frames per submit: the same network images per batch as ON, without the two kernels but with 16 frames to parse where ON
parses 8.  `kernels_share_of_batch` = 1 - ON / (that leg / 2) is therefore what copy + flip + merge cost MINUS the parser work the ensemble
saves: an upper bound only where it is positive, and negative where the parser's half weighs more than the kernels.  Method of tools/tiled_bench.py: clock ramp, then >= `--steps` timed submits with the pipes full, the last
result on the host; the legs alternate round by round in one process.

(b) Kernel part.  n = 8 at the same sizes: hp_hflip_u8c3 of 8 frames 432 x 368, hp_flip_merge on 16 conf maps [19, 46, 54] and on 16 paf maps
[38, 46, 54]; `--launches` launches back to back on the null stream + one synchronisation, wall time per launch, against hipMemcpyAsync
device-to-device of the bytes each kernel WRITES (n frames, n maps), measured the same way in the same rounds.  A launch of this size lasts about
as long as the host needs to issue it: the figures are the cost as a caller pays it, an upper bound of the device time; the default 50 000
launches make every timed window a few tenths of a second.  (The merge is timed in place on its own output, launch after launch: the values
converge to +-b, which changes nothing for a kernel whose time does not depend on the data.)
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
N = 8  # frames per submit, and the n of the kernel part


def pipeline_part(args) -> dict:
    import bench
    from hyperpose_amd import _lib, frontend
    from hyperpose_amd.engine import Model
    from hyperpose_amd.pipeline import Pipeline
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, (FRAME_H * 3 // 2 // 4, FRAME_W // 4), dtype=np.uint8)
    raw = np.repeat(np.repeat(small, 4, axis=0), 4, axis=1)  # blocky nv12 noise: the parser sees structure, not white noise
    bufs, strides = frontend.yuv_upload(frontend.yuv_planes(raw, "nv12", FRAME_W, FRAME_H), "nv12")
    images = (_lib.YuvImage * (2 * N))(*[frontend.yuv_image("nv12", [b.ptr for b in bufs], strides, FRAME_W, FRAME_H)] * (2 * N))
    out = {}
    for dtype in ("f32", "f16"):
        cfg = bench.config(1, dtype)
        pipes = cfg["pipes"]
        model = Model(cfg["arch"], cfg["w"], cfg["h"])
        weights = model.init_weights(cfg["seed"])
        make = lambda mb: Pipeline(model, weights, max_batch=mb, n_pipes=pipes, keep_ratio=True, max_frame_wh=(cfg["w"], cfg["h"]),  # noqa: E731
                                   parser=cfg["parser"], dtype=cfg["dtype"])
        p8, p16, p16on = make(N), make(2 * N), make(2 * N)
        p16on.set_flip_ensemble(True)
        legs = {"off_batch8": (p8, N), "on_batch16": (p16on, N), "off_batch16": (p16, 2 * N)}
        fps = {k: [] for k in legs}

        def timed(pl, n):
            def run(steps):
                for _ in range(steps):
                    if pl.in_flight == pl.n_pipes:
                        pl.collect()
                    pl.submit_yuv_images_raw(images, n, True)

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
            return round(n * done / (time.perf_counter() - t0), 1)

        for _ in range(args.rounds):
            for name, (pl, n) in legs.items():
                fps[name].append(timed(pl, n))
        rec = {name: {"frames_per_submit": legs[name][1], "frames_per_s_median": statistics.median(v), "frames_per_s_rounds": v} for name, v in fps.items()}
        off, on, off16 = (rec[k]["frames_per_s_median"] for k in ("off_batch8", "on_batch16", "off_batch16"))
        rec["on_over_off"] = round(on / off, 4)  # the expectation: 0.5
        # the same 16 network images per batch with and without flip + copy + merge, the plain leg with twice the frames to parse (see above)
        rec["kernels_share_of_batch"] = round(1.0 - on / (off16 / 2), 4)
        out[dtype] = rec
        print(f"{dtype}: off {off} frames/s (batch 8), on {on} (batch 16), off {off16} (batch 16); on / off = {rec['on_over_off']}, "
              f"1 - on / (off at batch 16 / 2) = {100 * rec['kernels_share_of_batch']:.1f} %", flush=True)
        for pl in (p8, p16, p16on):
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
    frames = _lib.DevBuf.from_numpy(rng.integers(0, 256, (2 * N, h, w, 3), dtype=np.uint8))
    frame_bytes = N * h * w * 3
    conf_perm, paf_perm, paf_sign = frontend.flip_tables_coco(19)
    cases = {}
    flip = lambda: frontend.hflip_u8c3(frames, frames.ptr.value + frame_bytes, w, h, N)  # noqa: E731
    cases["hflip_u8c3 8 x 432x368"] = (flip, frames, frame_bytes)
    for name, Cc, perm, sign in (("flip_merge conf 19x46x54", 19, conf_perm, np.ones(19, np.int8)), ("flip_merge paf 38x46x54", 38, paf_perm, paf_sign)):
        maps = _lib.DevBuf.from_numpy(rng.standard_normal((2 * N, Cc, mh, mw)).astype(np.float32))
        cases[name] = ((lambda maps=maps, Cc=Cc, perm=perm, sign=sign: frontend.flip_merge(maps, N, Cc, mh, mw, perm, sign)), maps, N * Cc * mh * mw * 4)
    out = {}
    for name, (kernel, buf, nbytes) in cases.items():
        def copy(buf=buf, nbytes=nbytes):
            if hip.hipMemcpyAsync(C.c_void_p(buf.ptr.value + nbytes), buf.ptr, nbytes, D2D, None) != 0:
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
    ap.add_argument("--skip-pipeline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flip_ensemble_bench.json"))
    args = ap.parse_args(argv)
    from hyperpose_amd import _lib
    _lib.init(0)
    rec = {"command": f"python tools/flip_ensemble_bench.py --steps {args.steps} --rounds {args.rounds} --launches {args.launches}" + (" --skip-pipeline" if args.skip_pipeline else ""),
           "kernel_method": f"n = {N}; {args.launches} launches back to back on the null stream + hp_device_synchronize, wall time / launches, min and median of "
                            f"{args.rounds} rounds, kernel and hipMemcpyAsync D2D (of the bytes the kernel writes) alternating; no profiler, nothing else on the device",
           "us_per_launch": kernel_part(args)}
    if not args.skip_pipeline:
        rec["pipeline_method"] = (f"BASELINE configs[1], 4 pipes, keep_ratio, device-resident nv12 {FRAME_W}x{FRAME_H}, 0.3 s ramp then >= {args.steps} timed submits, "
                                  f"median of {args.rounds} rounds, legs alternating: off at max_batch 8 ({N} frames per submit), on at max_batch 16 ({N} frames per "
                                  f"submit = 16 network images), off at max_batch 16 ({2 * N} frames per submit)")
        rec["pipeline_frames_per_s"] = pipeline_part(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
