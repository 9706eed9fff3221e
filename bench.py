#!/usr/bin/env python
"""bench.py — end-to-end FPS of the hot path on N MI355X (BASELINE.json metric).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config {0,1,2,3,4}] [--dtype {f32,f16}] [--scaling {weak,strong}] [--dump-outputs DIR]
                    [--full [--extra 1/f16,2/f32,...]]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

`--gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes itself under torch.distributed.run with N ranks
(one process per GPU, RCCL) and prints the ranks' ONE JSON line; under an external launcher it reads RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* as usual.

One "step" = one pass of the hot path over one batch.  The headline (`value`) is BASELINE.json configs[1] at the precision the
reference's engine defaults to, data_type::kFLOAT (include/hyperpose/operator/dnn/tensorrt.hpp:14-21,48 - `dtype: "f32"`, roofline
against the 157.3 TFLOP/s fp32 matrix pipe): Lightweight-OpenPose (MobilenetDilated backbone) + PAF parser, batch 8 @ 368x432 per GPU,
measured as SURVEY.md 8(d) / BASELINE.md 4.5 define it (the reference's loop, examples/operator_api_batched_images_paf.example.cpp:60-76: host
images in, humans out):
    u8 HWC frames in pinned HOST memory -> ONE H2D copy per batch -> (pre-processing fused into the first conv) -> conv stack on MFMA
    -> conf/paf fp32 maps in HBM -> PAF parser kernels on the network's OWN maps -> hp_human lists written to pinned host memory.
(Since round 6.  `value_resident_injected` is round 5's headline: frames already in HBM, the parser fed seeded synthetic maps with people;
`fps_dnn_output` the resident loop with the network's own maps.)  The fused fp16 engine (data_type::kHALF, the optional fast mode) is
`value_khalf` with its own `roofline_khalf`; `--dtype f16` makes it the headline.  Frames shard over GPUs with no steady-state collective;
the only collective is the one-time RCCL broadcast of the weight blob from rank 0 (outside the timed region).  `--scaling weak` (default):
every rank processes its own full batch per step; `--scaling strong`: the configuration's global batch is split contiguously over the ranks
(32 -> 4, 64 -> 8 frames per GPU).  `single_pipe_fps` / `operator_api_fps`: ONE batch in flight (a synchronous caller) through the
C ABI / through the C++ mirror's engine.inference + parser.process loop (examples/operator_api_bench.cpp).

A plain run (`--steps K --warmup W`) measures the headline alone: set-up, W untimed steps, 0.3 s of the same loop (also untimed: the
clocks settle), then ONE timed region of exactly K steps bracketed by barrier + torch.cuda.synchronize() on both sides, MAX over ranks:
`ms_per_step` = region / K.  `--min-seconds S` makes the region the smallest whole multiple R x K of the steps that lasts >= S s
(`steps_timed` = R x K).  `--dump-outputs DIR` then writes the humans the last timed step returned, and the conv stack's heat-maps of the
same seeded frames, to DIR/*.npy.

`--full` measures everything else as well (every region other than the headline's lasts >= 0.5 s unless --min-seconds is given): rank 0
prints ONE compact JSON line (<= 4 KB: `compact_line`; the driver parses the last stdout line) with the contract's keys, the headline's
`roofline` (dominant kernel: live per-launch time, both fractions, PMC traffic and the committed rocprofv3 average of the same kernel with
its source file) and `cpu_baseline`, and one small {value, ms_per_step, dtype, bound, frac} object per other workload (`--extra`; default
at N = 1: configs[1] at the other precision, then configs[0], [2], [3], [4] at both; at N > 1: configs[3], [4] strong-scaled).  EVERYTHING
else - full roofline objects with runner-up kernels, parser rooflines, single-pipe and host-fed legs, the clock / power samples of every
timed region, CPU-baseline samples - goes to `bench_detail.json` (named in the line as `detail`).  A plain run's line carries the
contract's keys and the headline's own figures only, and it writes no detail record.

Parser input: the networks have synthetic (random) weights, so their own heat-maps contain no people - they are dense noise, which is MORE
parser work per frame than a scene with people (thousands of sub-threshold-to-threshold maxima).  `value` parses those (the contract's
"network's own output"); the resident legs parse seeded synthetic heat-maps with several people per frame that are resident in HBM ("injected").
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F16_TFLOPS = 2500.0  # MI355X dense fp16/bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32_TFLOPS = 157.3   # v_mfma_f32_32x32x2_f32: the fp32 matrix pipe an HP_DTYPE_F32 (data_type::kFLOAT) engine computes on
# Independent engine+parser instances per GPU, one HIP stream each, batches round-robin over them.  Throughput depends
# on how those streams land on the runtime's hardware queues (measured on MI355X, tools/queue_probe.py, us/batch, config 1):
# 4 pipes on 2 queues (2+2) 606-617 | 3 pipes on 3 queues 657-667 | 6 pipes on 2 queues 668 | 4 pipes on 4 queues 790-820
# | 4 pipes on 1 queue 1030.  ROCm hands out hardware queues round-robin per created stream; every Pipe below creates an
# engine stream and then a parser stream, which puts the engine streams on alternating queues.
# compulsory parser bytes per frame (the network's output tensors read once; + <= 1.4 KB per human written)
PARSER_BYTES = {"paf": lambda h, w: 57 * (h // 8) * (w // 8) * 4, "ppn": lambda h, w: 855360 * (h // 32) * (w // 32) // 144,
                "pifpaf": lambda h, w: (17 * 5 + 19 * 9) * (((h - 1) // 8 + 1) * ((w - 1) // 8 + 1)) * 4}
PEAK_HBM_GBS = 8000.0
CONFIGS = {
    0: dict(label="configs[0]: TinyVGG-V2 + PAF parser, single 368x432 image (the reference's CPU-runnable plumbing case, src/fake)", arch="lw_openpose_vggtiny",
            w=432, h=368, batch=1, parser="paf", pipes=4, seed=20240, steps=400, people=(3,)),
    1: dict(label="configs[1]: Lightweight-OpenPose (MobilenetDilated) + PAF parser, batch 8 @ 368x432", arch="lw_openpose_mobilenet",
            w=432, h=368, batch=8, parser="paf", pipes=4, seed=20241, steps=400, people=(1, 2, 4, 8, 16, 3, 5, 6)),
    2: dict(label="configs[2]: OpenPose-COCO (VGG19) + PAF parser, batch 16 @ 432x768", arch="openpose_vgg19",
            w=768, h=432, batch=16, parser="paf", pipes=2, seed=20242, steps=24, people=(2, 4, 8, 16)),
    3: dict(label="configs[3]: PoseProposal ResNet-50 + NMS decoder, batch 32 @ 384x384", arch="pose_proposal_resnet50",
            w=384, h=384, batch=32, parser="ppn", pipes=8, seed=20243, steps=60, people=(1, 2, 3, 4)),
    4: dict(label="configs[4]: OpenPifPaf ResNet-50 + pif/paf seed-grow decoder, batch 64 @ 385x385", arch="pifpaf_resnet50",
            w=385, h=385, batch=64, parser="pifpaf", pipes=3, seed=20244, steps=16, people=(1, 2, 3, 4)),
}
# Steps per timed region when --steps is not given, per precision (fp32 engines are 3 - 6 x slower per step)
F32_STEPS = {0: 200, 1: 60, 2: 6, 3: 16, 4: 6}
F32_PIPES = {0: 4, 1: 4, 2: 2, 3: 4, 4: 2}
PEAK_F32S_TFLOPS = PEAK_F16_TFLOPS / 3  # HP_DTYPE_F32S: every fp32 product = three fp16 MFMA products (csrc/conv32_direct.hip): 833 TFLOP/s of fp32-equivalent work
PEAKS = {"f32": PEAK_F32_TFLOPS, "f16": PEAK_F16_TFLOPS, "f32s": PEAK_F32S_TFLOPS}
SECONDARY_MIN_S = 0.5  # minimum length of every timed region of --full other than the headline's
DTYPE_LABEL = {"f32": "f32", "f16": "f16", "f32s": "f32 (products as 3 exact f16xf16 MFMAs, fp32 accumulate)"}
DTYPE_LONG = {"f32": "f32 (data_type::kFLOAT, the reference's default: fp32 storage, v_mfma_f32_32x32x2_f32 products and sums; parsers fp32)",
              "f16": "f16 (data_type::kHALF: fp16 storage and MFMA products, fp32 accumulate; parsers fp32)",
              "f32s": "f32s (HP_DTYPE_F32S, opt-in: the kFLOAT engine - fp32 storage and accumulation - with the dense layers' products formed as "
                      "hi*hi + 2^-11 (hi*lo + lo*hi) on the fp16 matrix pipe, x = hi + 2^-11 lo split exactly into two fp16 numbers; parsers fp32)"}


def config(index: int, dtype: str) -> dict:
    """BASELINE.json configs[index] at one engine precision: 'f32' = data_type::kFLOAT, the reference engine's default
    (include/hyperpose/operator/dnn/tensorrt.hpp:14-21,48) and this bench's default; 'f16' = data_type::kHALF, the fused fp16 engine."""
    c = dict(CONFIGS[index])
    c["index"], c["dtype"], c["key"] = index, dtype, f"configs[{index}]/{dtype}"
    if dtype in ("f32", "f32s"):
        c["steps"], c["pipes"] = F32_STEPS[index], F32_PIPES[index]
    return c


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="steps K of the headline workload: its timed region is exactly K steps (unless "
                    "--min-seconds asks for a whole multiple of K lasting longer; reported as steps_timed)")
    ap.add_argument("--full", action="store_true", help="also measure everything beside the headline: the resident legs, rooflines, the CPU "
                    "baseline, clocks, the host-fed and operator-API legs and the other workloads (--extra), and write the detail record")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps write what the headline's last step returned "
                    "(humans, float32) and the conv stack's heat-maps of the same frames to DIR/<name>.npy")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", type=int, default=1, choices=[0, 1, 2, 3, 4, 5], help="headline workload: BASELINE.json configs index "
                    "(5 = old spelling of `--config 1 --dtype f32`)")
    ap.add_argument("--dtype", choices=("f32", "f16", "f32s"), default="f32", help="engine precision of the headline: f32 = data_type::kFLOAT, the "
                    "reference's default (default here too); f16 = data_type::kHALF, the fused fp16 engine")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak")
    ap.add_argument("--extra", default=None, help="comma-separated workloads also measured, as index/dtype (e.g. 1/f16,2/f32; '' = none)")
    ap.add_argument("--pipes", type=int, default=0, help="engine+parser pairs per GPU (0 = per config)")
    ap.add_argument("--min-seconds", type=float, default=None, help="minimum length of every timed region (default: none for the headline's, "
                    f"which is then exactly --steps steps, and {SECONDARY_MIN_S} s for every other region of --full)")
    ap.add_argument("--detail", default=None, help="where the full record goes (default: bench_detail.json next to bench.py, and "
                    "gpurun_out/bench_detail.json when that directory exists)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-from-host", action="store_true")
    ap.add_argument("--no-dnn-output", action="store_true", help="skip the second timed phase (parser fed by the network's own heat-maps)")
    ap.add_argument("--no-clocks", action="store_true", help="do not sample sclk / power during the timed regions")
    ap.add_argument("--no-operator-api", action="store_true", help="do not run the C++ operator-API loop (a child process: under rocprofv3 its half-batch "
                    "launches would be averaged into the per-kernel summaries)")
    args = ap.parse_args(argv)
    if args.config == 5:
        args.config, args.dtype = 1, "f32"
    return args


# ------------------------------------------------------------------------------------------------ multi-GPU launch
def respawn(n_gpus: int) -> int:
    """`python bench.py --gpus N` without a launcher: run N ranks of this file under torch.distributed.run (RCCL over xGMI,
    rendezvous on 127.0.0.1) and hand their stdout (rank 0's JSON line) through."""
    from hyperpose_amd import _lib
    have = _lib.lib().hp_device_count()
    if have < n_gpus:
        print(f"bench.py: --gpus {n_gpus} but only {max(have, 0)} HIP device(s) are visible", file=sys.stderr)
        return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def rank_plan(cfg_batch: int, scaling: str, rank: int, world: int):
    """(frames this rank processes per step, global frames per step).  weak: every rank its own full batch; strong: the
    configuration's batch split contiguously (hyperpose_amd.dist.shard)."""
    from hyperpose_amd import dist as hd
    if scaling == "strong":
        _, cnt = hd.shard(cfg_batch, rank, world)
        return cnt, cfg_batch
    return cfg_batch, cfg_batch * world


# ------------------------------------------------------------------------------------------------ one workload
class Pipe:
    """engine + parser sharing one stream; at most one batch in flight per pipe."""

    def __init__(self, cfg, model, weights, injected, batch):
        from hyperpose_amd.engine import Engine
        from hyperpose_amd import parser as P
        from hyperpose_amd._lib import HpError
        self._HpError = HpError
        self.kind, self.batch = cfg["parser"], batch
        self.eng = Engine.from_model(model, weights, max_batch=batch, dtype=cfg.get("dtype", "f16"))
        self.stream = self.eng.stream
        outs = self.eng.outputs  # sorted by name = the parsers' argument order
        if self.kind == "paf":
            self.par = P.Paf(max_batch=batch)
            (_, self.s0, d0), (_, self.s1, d1) = outs
            self.dnn = (d0, d1)
        elif self.kind == "ppn":
            self.par = P.PoseProposal((cfg["w"], cfg["h"]), max_batch=batch)
            self.dnn = [d for _, _, d in outs]
            self.s0 = outs[0][1]
            e = outs[6][1]
            nn = int(round((e[0] // 17) ** 0.5))
            self.s1 = (17, nn, nn, e[1], e[2])
        else:
            self.par = P.PifPaf(cfg["h"], cfg["w"], max_batch=batch)
            self.dnn = (outs[0][2], outs[1][2])
            self.s0 = outs[1][1]  # pif [85, fh, fw]
        self.inj = injected
        self.busy = self.eng_only = False
        # frames the device decoders handed to the host statements (PoseProposal / PifPaf: hp_*_decode_flags > 0) and batches in which a
        # fixed-capacity list of the PAF parser overflowed (HP_ERR_CAPACITY; the reference's vectors are unbounded) - reported, never hidden
        self.declined_frames = self.capacity_truncations = self.frames_parsed = 0
        self.last = None  # the humans of the last batch collected (--dump-outputs)

    def submit(self, frames_dev, injected: bool, engine: bool = True, parser: bool = True):
        n = self.batch
        if engine:
            self.eng.enqueue_u8(frames_dev, n)
        if not parser:
            self.eng_only = True  # collect() waits for the stream
            return
        src = self.inj if injected else self.dnn
        if self.kind == "paf":
            self.par.enqueue(src[0], src[1], n, self.s0, self.s1, stream=self.stream)
        elif self.kind == "ppn":
            self.par.enqueue(src, n, self.s0, self.s1, stream=self.stream)
        else:
            self.par.enqueue(src[0], src[1], n, self.s0[1], self.s0[2], stream=self.stream)
        self.busy = True

    def collect(self):
        if self.eng_only:
            self.eng.synchronize()
            self.eng_only = False
        if not self.busy:
            return 0
        self.busy = False
        try:
            humans = self.par.collect()
        except self._HpError as e:
            if e.code != -3:  # HP_ERR_CAPACITY: counted; anything else is a failure of the run
                raise
            self.capacity_truncations += 1
            return 0
        self.frames_parsed += self.batch
        self.last = humans
        if self.kind != "paf":
            self.declined_frames += int(sum(1 for f in self.par.decode_flags(self.batch) if f > 0))
        return sum(len(h) for h in humans)


def run_loop(pipes, frames_dev, steps, injected):
    n_humans = 0
    for i in range(steps):
        p = pipes[i % len(pipes)]
        n_humans += p.collect()
        p.submit(frames_dev, injected)
    for p in pipes:
        n_humans += p.collect()
    return n_humans


def synth_frames(cfg, batch, rank):
    """The u8 frames of synth_inputs alone (the same arrays: they are drawn first from the same generator)."""
    from hyperpose_amd import synth
    return synth.images_u8(synth.rng_for(cfg["index"], salt=rank), batch, cfg["h"], cfg["w"])


def synth_inputs(cfg, batch, rank):
    """Per-rank seeded synthetic inputs of one workload: u8 frames + the parser's injected tensors (host numpy)."""
    from hyperpose_amd import synth
    idx = cfg["index"]
    rng = synth.rng_for(idx, salt=rank)
    frames = synth.images_u8(rng, batch, cfg["h"], cfg["w"])
    if cfg["parser"] == "paf":
        conf, paf, _ = synth.paf_maps(rng, batch, cfg["h"] // 8, cfg["w"] // 8, people=cfg["people"])
        maps = [conf, paf]
    elif cfg["parser"] == "ppn":
        maps = synth.ppn_maps(rng, batch, net=cfg["w"], grid=cfg["w"] // 32, people=cfg["people"])
    else:
        f = (cfg["w"] - 1) // 8 + 1
        maps = list(synth.pifpaf_maps(rng, batch, f, f, people=cfg["people"]))
    return frames, maps


def cpu_baseline(cfg, maps, budget_s=8.0):
    """The reference's CPU parser on this host's cores with the reference's shipping flags (-Ofast) and its own parallel
    model: one parser replica per pool thread, frames round-robin (include/hyperpose/utility/thread_pool.hpp:21,
    stream.hpp:139-144).  All three parsers are the reference's own sources compiled in oracle/_ref ("reference"); for PAF
    (src/paf.cpp + src/post_process.hpp behind the container shims of oracle/shim) the two OpenCV calls are the scalar
    restatements of oracle/paf_oracle.cpp, i.e. without OpenCV's SIMD kernels - the sample says so."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import loader
    ncpu = os.cpu_count() or 1
    threads = max(1, min(14, ncpu + 2, ncpu))
    kind = cfg["parser"]
    nb = maps[0].shape[0]
    if kind == "paf":
        if loader.have_ref_paf(fast=True):
            def one(i):
                return len(loader.ref_paf_process(maps[0][i], maps[1][i], fast=True, debug=False)[0])
            what, tag = ("reference src/paf.cpp + src/post_process.hpp compiled in oracle/_ref (its two OpenCV calls = scalar "
                         "restatements, no OpenCV SIMD), -Ofast -march=x86-64-v3"), "reference"
        else:
            def one(i):
                return len(loader.paf_process(maps[0][i], maps[1][i], fast=True)[0])
            what, tag = "restated reference PAF parser (no OpenCV SIMD), -Ofast -march=x86-64-v3", "port"
    elif kind == "ppn":
        if loader.ref_lib(fast=True) is None:
            return None
        def one(i):
            return len(loader.ref_ppn_process([m[i] for m in maps], net_w=cfg["w"], net_h=cfg["h"], fast=True))
        what, tag = "reference src/pose_proposal.cpp compiled in oracle/_ref, -Ofast", "reference"
    else:
        if loader.ref_lib(fast=True) is None:
            return None
        def one(i):
            return len(loader.ref_pifpaf_process(maps[0][i], maps[1][i], net_h=cfg["h"], net_w=cfg["w"], fast=True))
        what, tag = "reference src/pifpaf.cpp + src/pifpaf_decoder compiled in oracle/_ref, -Ofast", "reference"
    one(0)  # warm / build
    t0 = time.perf_counter()
    one(0)
    lat = time.perf_counter() - t0
    frames = int(max(threads * 2, min(400, budget_s / max(lat, 1e-4) * threads)))
    idx = [i % nb for i in range(frames)]
    with ThreadPoolExecutor(threads) as ex:
        t0 = time.perf_counter()
        list(ex.map(one, idx))
        dt = time.perf_counter() - t0
    return {"value": round(frames / dt, 2), "unit": "frames/s (parser only; the reference's DNN stage is TensorRT and has no CPU path)",
            "cores": threads, "host_cores": ncpu, "kind": tag,
            "sample": f"{frames} injected heat-map frames of this workload (its {nb} frames cycled), {threads} threads on a host with "
                      f"{ncpu} logical cores, single-thread latency {lat * 1e3:.2f} ms/frame, {what}"}


class HostFed:
    """The stream operator's device pipeline (hp_pipeline_*) fed from pinned HOST memory: per batch one H2D copy (network-sized frames) or per-frame
    copies + the resize kernel (camera-sized frames), the conv stack, the parser on the network's OWN maps, humans back on the host.  `n_pipes`
    engine + parser pairs, batches round-robin over them, results in submission order."""

    def __init__(self, model, weights, cfg, batch, pipes, frame_wh, keep_ratio, frames_u8=None):
        import ctypes as C

        from hyperpose_amd import _lib
        from hyperpose_amd.pipeline import Pipeline
        w_, h_ = frame_wh
        self.nbytes, self.batch = w_ * h_ * 3, batch
        self._lib = _lib.lib()
        self.host = C.c_void_p()
        _lib.check(self._lib.hp_malloc_host(C.byref(self.host), C.c_size_t(self.nbytes * batch)))
        if frames_u8 is not None and frames_u8.shape[1:] == (h_, w_, 3):
            src = np.ascontiguousarray(frames_u8[:batch]).reshape(-1)
        else:
            src = np.random.default_rng(7).integers(0, 256, self.nbytes * batch, dtype=np.uint8)
        C.memmove(self.host, src.ctypes.data, src.nbytes)
        self.ptrs = (C.POINTER(C.c_uint8) * batch)(*[C.cast(self.host.value + i * self.nbytes, C.POINTER(C.c_uint8)) for i in range(batch)])
        self.ws, self.hs = (C.c_int * batch)(*([w_] * batch)), (C.c_int * batch)(*([h_] * batch))
        self.pl = Pipeline(model, weights, max_batch=batch, n_pipes=pipes, keep_ratio=keep_ratio, max_frame_wh=frame_wh, parser=cfg["parser"],
                           dtype=cfg.get("dtype", "f16"))
        self.humans = 0
        self.last = None  # the humans of the last batch collected: the last step's once drained (--dump-outputs)

    def _collect(self):
        self.last = self.pl.collect()
        self.humans += sum(len(h) for h in self.last)

    def run(self, n):
        """n more steps; the pipes stay full (a drain after every few steps would time the fill and the drain, not the pipeline)"""
        pl = self.pl
        for _ in range(n):
            if pl.in_flight == pl.n_pipes:
                self._collect()
            pl.submit_ptrs(self.ptrs, self.ws, self.hs, self.batch)

    def drain(self):
        while self.pl.in_flight:
            self._collect()

    def close(self):
        self.drain()
        self.pl.close()
        self._lib.hp_free_host(self.host)


def _host_pipeline_rate(model, weights, cfg, batch, pipes, steps, frame_wh, keep_ratio, min_s=0.6):
    hf = HostFed(model, weights, cfg, batch, pipes, frame_wh, keep_ratio)
    # clock ramp (0.3 s untimed, drained), then whole multiples of `chunk` steps until at least `min_s` have been timed - independent of
    # --steps; the timed region starts with empty pipes and ends when the last result is on the host
    chunk = max(2 * pipes, 4)
    t_ramp = time.perf_counter()
    while time.perf_counter() - t_ramp < 0.3:
        hf.run(chunk)
    hf.drain()
    done = 0
    t0 = time.perf_counter()
    while done < steps or time.perf_counter() - t0 < min_s:
        hf.run(chunk)
        done += chunk
    hf.drain()
    dt = time.perf_counter() - t0
    nbytes = hf.nbytes
    hf.close()
    return batch * done / dt, nbytes * batch, done


def from_host(model, weights, cfg, batch, pipes, steps=8, frame_wh=(1280, 720)):
    """Camera-sized frames: per batch H2D copies, non_scaling_resize on the device, conv stack, parser, resume_ratio - the GPU form of
    hyperpose::stream."""
    fps, nb, steps = _host_pipeline_rate(model, weights, cfg, batch, pipes, steps, frame_wh, True)
    return {"value": round(fps, 1), "unit": "frames/s", "steps": steps,
            "what": f"{frame_wh[0]}x{frame_wh[1]} BGR frames in pinned host memory -> H2D ({nb / 1e6:.1f} MB per batch) -> "
                    "non_scaling_resize on the GPU -> conv stack -> parser (the network's own heat-maps) -> resume_ratio -> humans on the host"}


def operator_api(cfg, batch, seconds=1.5):
    """The reference's operator-API loop (examples/operator_api_batched_images_paf.example.cpp:60-76: engine.inference(std::vector<cv::Mat>) then
    parser.process(packet[0], packet[1]) per frame, ONE batch in flight, a synchronous caller) through the C++ mirror headers: the host program
    examples/operator_api_bench.cpp, built by hyperpose_amd.build.build_operator_bench (g++).  PAF workloads only."""
    from hyperpose_amd import build as hb
    if cfg["parser"] != "paf" or not os.path.exists(hb.BENCH_BIN):
        return None
    try:
        out = subprocess.run([hb.BENCH_BIN, cfg["arch"], str(cfg["w"]), str(cfg["h"]), str(batch), str(seconds), "f16" if cfg["dtype"] == "f16" else "f32"],
                             capture_output=True, text=True, timeout=120)
        return json.loads(out.stdout.strip().splitlines()[-1])
    except (OSError, ValueError, IndexError, subprocess.SubprocessError) as e:
        return {"error": str(e)[:200]}


def kernel_label(tile: int):
    """(substring of the kernel symbol as rocprofv3 prints it, human-readable label) for a profile row's `tile` code
    (conv_kernels.hpp: conv_mfma_tile; engine.cpp: hp_engine_profile)."""
    sep = {7: ("sepconv_small_kernel<32,1,2>", "32-channel separable block, all channels of an 8x8 tile in LDS"),
           1: ("sepconv_small_kernel<", "separable block -> 128 channels, all channels of an 8x8 tile in LDS"),
           2: ("sepconv_small_kernel<", "separable block -> 128 channels, stride 2, all channels of a tile in LDS"),
           3: ("sepconv_slot_kernel<2,1,2,1,128,64>", "separable block 128 -> 256, stride 2, half-CU form"),
           4: ("sepconv_slot_kernel<1,2,1,1,256,64>", "separable block 256 -> 256, half-CU form"),
           5: ("sepconv_pipe3_kernel<1,false,true>", "separable block 256 / 512 -> 512: 12x8 pixels x all 512 output channels per block, eight wavefronts; per 64-channel "
               "chunk the depthwise taps of chunk k+1 are issued between the pointwise MFMAs of chunk k in the SAME wavefront (one stream of 24 slots)"),
           6: ("sepconv_pipe3_kernel<2,false,true>", "separable block 512 -> 512, dilation 2, same form"),
           20: ("sepconv_pair_kernel<32,64,128>", "the stem's separable blocks 32 -> 64 and 64 -> 128 (stride 2) in one launch, the 64-channel "
                "tensor between them in LDS only")}
    chain = {1: "false,0", 2: "false,1", 3: "false,2", 10: "true,0", 13: "true,3"}
    if tile >= 39000000:
        kt, bn = (tile - 39000000) // 1000, tile % 1000
        return (f"conv32_wk_kernel<{kt},{bn}>", f"conv32_wk_kernel<K={kt},BN={bn}> (fp32 1x1 layer with {kt} input channels on v_mfma_f32_16x16x4_f32: 64 cout x {bn} pixels per block, weights, "
                "pixels (all K), residual and bias requested at once, no K-step barriers, whole-line row-major stores through a per-wavefront LDS slab)")
    if tile >= 37000000:
        hid, c2 = (tile - 37000000) // 100, tile % 100
        # (round 6: two heads that read the same tensor run as ONE grid, conv32_head_pair_kernel<TM2a,TM2b>; a lone head as conv32_head_kernel<TM2>.
        # The key matches whichever ONE of them a trace holds; a trace with both forms is ambiguous and quotes no committed duration)
        return ("conv32_head_", f"conv32_head_kernel (fp32 two-layer head in one launch: 1x1 128 -> {hid} relu -> 1x1 {hid} -> {c2}, 32 pixels per block, "
                "the hidden tile's accumulator registers are the second layer's B operand; the heat-map and PAF heads of a stage share one grid)")
    if tile >= 35000000:
        mw = tile % 1000
        if tile // 1000 == 35005:
            return ("conv32_winograd3_kernel", "conv32_winograd3_kernel (opt-in HP_WINO_F33=1: fp32 3x3 stride-1 convolution in Winograd's F(3x3,3x3) form on v_mfma_f32_16x16x4_f32: 25 MFMA products "
                    "per 3x3 output tile and channel pair instead of 81; 64 cout x 24x6 px per block)")
        # (third template argument: 16-tile MFMA columns per block - 2 = the 16 x 8-pixel form of every pipelined run, 1 = the 8 x 8-pixel form a caller with one batch in flight gets)
        return (f"conv32_winograd_kernel<{mw},{'true' if mw == 4 else 'false'},2>", f"conv32_winograd_kernel<MW={mw}> (fp32 3x3 stride-1 convolution in Winograd's F(2x2,3x3) form on v_mfma_f32_16x16x4_f32: 16 MFMA "
                f"products per output tile and channel pair instead of 36; {16 * mw} cout x 16x8 px per block, input transform through LDS, U = G g Gt in fragment order from L2; "
                "flops = the MFMA work issued)")
    if 35000000 > tile >= 33000000 and (tile // 100000) % 10:  # a depthwise 3 x 3 fused in front of the 1 x 1 layer
        split, dil, mw = tile < 34000000, (tile // 100000) % 10, tile % 1000
        return (f"conv32_direct_kernel<{'true' if split else 'false'},1,64,{mw},{dil}>", f"conv32_direct_kernel<{'split' if split else 'fp32'},KS=1,MW={mw},DWD={dil}> (separable block in one launch: "
                f"the depthwise 3x3 (dilation {dil}) computed from its input tile in LDS straight into the tile the 1x1 layer's MFMAs read; {(64 if split else 32) * mw} cout x 8x8 px per block)")
    if 35000000 > tile >= 34000000:
        ks, mw = (tile - 34000000) // 1000, tile % 1000
        return (f"conv32_direct_kernel<false,{ks},{64 if ks == 1 else 32},{mw},0>", f"conv32_direct_kernel<fp32,KS={ks},MW={mw}> (exact fp32 products on v_mfma_f32_32x32x2_f32: "
                f"{32 * mw} cout x 8x8 px per block, {2 * mw} wavefronts of one 32x32 tile, the chunk's halo tile in LDS once for all taps, weights in fragment order from L2, no barrier per K-step)")
    if tile >= 33000000:
        ks, mw = (tile - 33000000) // 1000, tile % 1000
        return (f"conv32_direct_kernel<true,{ks},{64 if ks == 1 else 32},{mw},0>", f"conv32_direct_kernel<split,KS={ks},MW={mw}> (fp32 convolution with every product formed as three exact "
                f"fp16 x fp16 MFMA products: {64 * mw} cout x 8x8 px per block, split halo tile in LDS, split weights in fragment order from L2)")
    if tile >= 32000000:
        v = tile - 32000000
        rows, v = v >= 400000, v % 400000
        bm, bn = v // 1000, v % 1000
        wm, wn = (1, 4) if (bm, bn) == (64, 128) else (2, 2)
        if bn == 160:
            return ("conv32_t16_kernel<160,2>", "conv32_t16_kernel<BN=160> (fp32 implicit GEMM on v_mfma_f32_16x16x4_f32: 64 cout x 160 pixels per block = ONE round of "
                    "four blocks per CU where 64 x 128 tiles need a round and a bit; 2 x 2 wavefronts of 32 x 80, A and B staged through swizzled LDS, K-steps of 16 channels)")
        if bn == 176:
            return ("conv32_t16_kernel<176,1>", "conv32_t16_kernel<BN=176> (fp32 implicit GEMM on v_mfma_f32_16x16x4_f32: 64 cout x 176 pixels per block = ONE round of "
                    "four blocks per CU where 64 x 160 tiles are a few blocks more than the chip's 1024 slots; four wavefronts of 16 x 176, swizzled LDS, K-steps of 16 channels)")
        return (f"conv32_kernel<{bm},{bn},{wm},{wn},{'true' if rows else 'false'}>", f"conv32_kernel<BM={bm},BN={bn}> (fp32 implicit GEMM on v_mfma_f32_32x32x2_f32: {bm} cout x {bn} pixels per block, "
                f"A and B staged through LDS in fp32, K-steps of 16 channels, {'row-major' if rows else 'lane = pixel'} epilogue)")
    if tile >= 9000000:
        v = tile - 9000000
        m, pj, mr, a3 = v // 1000 * 64, v // 100 % 10, v // 10 % 10 * 64, v % 10
        own, pj = pj >= 2, pj % 2
        what = (f"{'own 1x1 reduction -> ' if own else ''}{'3x3 -> ' if a3 else ''}1x1 {m} -> {4 * m} + {'projection' if pj else 'shortcut'}"
                f"{f' -> 1x1 {4 * m} -> {mr} of the next block' if mr else ''} in one launch, 8x8 pixels per block, intermediates in LDS")
        if m == 64:
            t = lambda x: "true" if x else "false"
            return (f"bottleneck64_kernel<{mr},{t(a3)},{t(pj)},{t(own)}>", "bottleneck64_kernel (" + what + ")")
        if a3:
            return (f"bottleneck_kernel<128,{mr},true>", "bottleneck_kernel (" + what + ")")
        return (f"bottleneck128_kernel<{mr}>", "bottleneck128_kernel (" + what + ")")
    if tile >= 7000000:
        v = tile - 7000000
        return (f"conv_chain_kernel<{chain.get(v, '')},", "conv_chain_kernel ([1x1 ->] 3x3 -> 3x3 [+ residual] on 128 channels in one launch: 8x8 output pixels x all "
                "128 channels per block, intermediates in LDS, weights in MFMA-fragment order straight from L2)")
    if tile >= 6000000 and tile % 1000 in (9, 25, 49):
        v = tile - 6000000
        cin, taps = v // 1000, v % 1000
        ks = int(round(taps ** 0.5))
        ck, nbuf = (128, 1) if cin == 128 else (64, 1 if cin == 64 else 2)
        return (f"conv_direct_kernel<{ks},{ck},{nbuf}>",
                f"conv_direct_kernel<KS={ks},CK={ck},NBUF={nbuf}> ({ks}x{ks} taps, {cin} input channels in {cin // ck} chunk(s); 8 wavefronts, 128 cout x 16x12 px "
                "per block, halo tile of a chunk in LDS for all taps, weights in MFMA-fragment order straight from L2)")
    if tile >= 6000000:
        return ("mlp_head", "mlp_head(_pair)_kernel (1x1 K1 -> 512 relu -> 1x1 512 -> 19 | 38, hidden tensor in registers)")
    if 5200000 <= tile < 5300000:
        tm, ntp = (tile - 5200000) // 1000, tile % 1000
        return (f"conv1x1_big_kernel<{tm},{ntp}>", f"conv1x1_big_kernel<TM={tm},NTP={ntp}> (pixel-block GEMM: {32 * ntp} pixels x {128 * tm} output channels per block, "
                "weights from L2 in fragment order, activations through producer wavefronts + LDS)")
    if 5100000 <= tile < 5200000:
        return ("conv1x1_small_kernel", "conv1x1_small_kernel (64 pixels x all input channels in LDS, fragment-ordered weights from L2)")
    if tile >= 5000000:
        return ("conv3x3_direct_kernel<128,", "conv3x3_direct_kernel<CIN=128> (64 cout x 16x12 px tile, input halo tile in LDS, weights in MFMA-fragment order straight from L2)")
    if tile >= 4000000:
        return sep.get(tile - 4000000, ("sepconv", "fused depthwise 3x3 + pointwise 1x1"))
    return (f"conv_mfma_kernel<{tile // 1000},{tile % 1000},", f"conv_mfma_kernel<BM={tile // 1000},BN={tile % 1000}> (implicit GEMM, A and B staged through LDS)")


def pmc_traffic(symbol_key: str, tag: str):
    """HBM bytes per launch of the kernel from the committed rocprofv3 PMC passes (profiles/<round>_pmc_traffic*.json):
    newest round first; kernel names compared with blanks removed."""
    import glob
    want = symbol_key.replace(" ", "")
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_traffic{tag}.json")), reverse=True):
        try:
            pmc = json.load(open(path))["kernels"]
        except (OSError, KeyError, ValueError):
            continue
        for name, d in pmc.items():
            if want in name.replace(" ", "") and "hbm_bytes_per_launch" in d:
                return round(d["hbm_bytes_per_launch"]), os.path.basename(path)
    return None, None


def pmc_mfma_busy(symbol_key: str, tag: str):
    """SQ_VALU_MFMA_BUSY_CYCLES / (4 SIMDs x SQ_BUSY_CU_CYCLES) of the kernel from the newest committed rocprofv3 SQ pass
    (profiles/<round>_pmc_sq<tag>.json, tools/collect_profiles.sh): (fraction, wait_inst_any fraction, file name) - the counter the north
    star asks for next to the roofline fraction.  Not measured in this run."""
    import glob
    want = symbol_key.replace(" ", "")
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_pmc_sq{tag}.json")), reverse=True):
        try:
            pmc = json.load(open(path))["kernels"]
        except (OSError, KeyError, ValueError):
            continue
        hits = [d for name, d in pmc.items() if want in name.replace(" ", "")]
        if len(hits) == 1 and "mfma_busy_frac" in hits[0]:
            return round(hits[0]["mfma_busy_frac"], 4), round(hits[0].get("SQ_WAIT_INST_ANY_share_of_wave_cycles", 0.0), 4), os.path.basename(path)
        return None, None, os.path.basename(path)
    return None, None, None


def rocprof_avg_us(symbol_key: str, tag: str):
    """Average duration of the kernel in the NEWEST committed `rocprofv3 --kernel-trace --stats` summary of this bench command
    (profiles/<round>_kernel_stats<tag>.csv): (us, file name), or (None, file name) unless the key names EXACTLY ONE row of that file -
    an ambiguous or missing key (a renamed kernel, a template instance the key does not pin down) must not produce a number."""
    import csv
    import glob
    want = symbol_key.replace(" ", "")
    paths = sorted(glob.glob(os.path.join(ROOT, "profiles", f"r*_kernel_stats{tag}.csv")), reverse=True)
    if not paths:
        return None, None
    try:
        with open(paths[0], newline="") as f:
            hits = [row for row in csv.DictReader(f) if want in row.get("Name", "").replace(" ", "")]
        if len(hits) == 1:
            return float(hits[0]["AverageNs"]) / 1e3, os.path.basename(paths[0])
    except (OSError, KeyError, ValueError):
        pass
    return None, os.path.basename(paths[0])


RIDGE_FLOP_PER_BYTE = 2500.0e12 / 8000.0e9  # 312.5: below it a kernel's binding roof is HBM, above it the matrix pipe


def profile_tag(cfg) -> str:
    """suffix of this workload's committed rocprofv3 summaries: profiles/<round>_kernel_stats<tag>.csv, <round>_pmc_traffic<tag>.json"""
    i = cfg["index"]
    if cfg["dtype"] == "f32":
        return f"_config{i}_fp32"
    if cfg["dtype"] == "f32s":
        return f"_config{i}_fp32s"
    return "" if i == 1 else f"_config{i}"


def roofline(pipe, batch, cfg, frames_dev=None):
    """Per-launch timestamps on the engine stream with the schedule run in order (hp_engine_profile_sequence: every kernel sees the
    cache state of a real inference, which is what rocprofv3's per-kernel averages over this bench see too).  achieved = algorithmic
    FLOPs (or bytes) of the dominant kernel's launches / their summed duration.  `back_to_back_us` is the same kernel re-launched 20
    times in a row (weights warm in L2) for comparison."""
    peak_tflops = PEAKS[cfg["dtype"]]
    small = cfg["index"] in (0, 1)
    iters = 20 if small else 4
    # the median of three passes per step: one pass of 4 iterations now and then caught a stall (a 160 us kernel reported at 456 us on one box,
    # the workload's own throughput unchanged) and the roofline object quoted it
    passes = [pipe.eng.profile(batch, iters=iters, in_sequence=True) for _ in range(3)]
    prof = passes[0]
    for k, p0_ in enumerate(prof):
        p0_["ms"] = sorted(ps[k]["ms"] for ps in passes)[1]
    warm = pipe.eng.profile(batch, iters=iters) if small else None
    mfma = [p for p in prof if p["tile"] != 0]
    by_tile = {}
    for p in mfma:
        d = by_tile.setdefault(p["tile"], {"ms": 0.0, "flops": 0.0, "bytes": 0.0, "n": 0})
        d["ms"] += p["ms"]
        d["flops"] += p["flops"]
        d["bytes"] += p["bytes"]
        d["n"] += 1
    dom_tile, dom = max(by_tile.items(), key=lambda kv: kv[1]["ms"])
    tot_ms = sum(p["ms"] for p in prof)
    mfma_ms = sum(p["ms"] for p in mfma)
    mfma_fl = sum(p["flops"] for p in mfma)
    tflops = dom["flops"] / (dom["ms"] * 1e-3) / 1e12
    gbs = dom["bytes"] / (dom["ms"] * 1e-3) / 1e9   # ALGORITHMIC bytes of the launches (input + output + weights once, engine.cpp st.bytes)
    intensity = dom["flops"] / dom["bytes"]
    ridge = peak_tflops * 1e12 / (PEAK_HBM_GBS * 1e9)
    bound = "mfma" if intensity >= ridge else "hbm"
    frac_mfma, frac_hbm = tflops / peak_tflops, gbs / PEAK_HBM_GBS
    key, label = kernel_label(dom_tile)
    tag = profile_tag(cfg)
    traffic, src = pmc_traffic(key, tag)
    prof_us, prof_src = rocprof_avg_us(key, tag)
    if 39000000 > dom_tile >= 37000000:
        prof_us, prof_src = None, None  # (a pair launch's duration covers two heads: not this step's)
    busy, wait_any, busy_src = pmc_mfma_busy(key, tag)
    out = {
        # the roof that binds THIS kernel: its arithmetic intensity against the ridge (peak FLOP/s of the engine's matrix pipe / 8 TB/s);
        # `achieved` / `peak` / `frac` are quoted on that roof, both fractions are given below
        "bound": bound,
        "achieved": round(tflops, 2) if bound == "mfma" else round(gbs, 1),
        "peak": peak_tflops if bound == "mfma" else PEAK_HBM_GBS,
        "unit": "TFLOP/s" if bound == "mfma" else "GB/s",
        "frac": round(frac_mfma if bound == "mfma" else frac_hbm, 4),
        "intensity_flop_per_byte": round(intensity, 1), "ridge_flop_per_byte": round(ridge, 2), "mfma_peak_tflops": peak_tflops,
        "frac_mfma": round(frac_mfma, 4), "achieved_tflops": round(tflops, 2),
        "frac_hbm": round(frac_hbm, 4), "achieved_gbs": round(gbs, 1),
        # the largest fraction of the MFMA peak this kernel could reach at 8 TB/s given its intensity (1 when it is right of the ridge)
        "mfma_frac_ceiling_at_hbm_peak": round(min(1.0, intensity / ridge), 4),
        "traffic": traffic, "traffic_source": src,
        # the matrix pipe's own busy counter for this kernel, from the committed rocprofv3 SQ pass of the same bench command (not this run)
        "mfma_busy": busy, "wait_inst_any": wait_any, "mfma_busy_source": busy_src,
        "kernel": label, "kernel_symbol": key,
        "launches_per_step": dom["n"], "avg_launch_us": round(dom["ms"] / dom["n"] * 1e3, 2),
        "flops_per_launch": round(dom["flops"] / dom["n"]), "algorithmic_bytes_per_launch": round(dom["bytes"] / dom["n"]),
        # a Winograd F(2x2,3x3) kernel issues 16 MFMA products where the layer's algorithmic (direct-form) count has 36: `frac` above is of the
        # ALGORITHMIC flops (the contract's definition; it may pass what the pipe could do in direct form), this is the pipe's own utilisation
        **({"frac_mfma_issued": round(frac_mfma * 16 / 36, 4), "mfma_issued_flops_per_launch": round(dom["flops"] / dom["n"] * 16 / 36)} if 37000000 > dom_tile >= 35000000 else {}),
        # NOT measured in this run: the kernel's average duration in the newest COMMITTED rocprofv3 kernel trace of `bench.py --config N
        # --dtype D --pipes 1` (the tracer adds ~1 us per launch) and this run's FLOPs over it - for the reader who recomputes the fraction
        # from profiles/; null unless the kernel's name matches exactly one row of that file
        "committed_profile": {"source": prof_src, "avg_launch_us": None if prof_us is None else round(prof_us, 2),
                              "frac_mfma": None if prof_us is None else round(dom["flops"] / dom["n"] / (prof_us * 1e-6) / 1e12 / peak_tflops, 4),
                              "frac_hbm": None if prof_us is None else round(dom["bytes"] / dom["n"] / (prof_us * 1e-6) / 1e9 / PEAK_HBM_GBS, 4)},
        "all_mfma_convs": {"achieved": round(mfma_fl / (mfma_ms * 1e-3) / 1e12, 2), "frac": round(mfma_fl / (mfma_ms * 1e-3) / 1e12 / peak_tflops, 4),
                           "ms_per_step": round(mfma_ms, 4), "launches_per_step": len(mfma)},
        "serial_layer_ms_per_step": round(tot_ms, 4),
        "non_mfma_ms_per_step": round(tot_ms - mfma_ms, 4),
    }
    # the kernel with the second-largest share (on configs[1]/f16 the 512-output separable block and the 128-channel chain swap places
    # between runs / boxes): always in the detail record
    rest = sorted(((t, d) for t, d in by_tile.items() if t != dom_tile), key=lambda kv: -kv[1]["ms"])
    if rest:
        t2, d2 = rest[0]
        tf2, gb2, in2 = d2["flops"] / (d2["ms"] * 1e-3) / 1e12, d2["bytes"] / (d2["ms"] * 1e-3) / 1e9, d2["flops"] / d2["bytes"]
        out["runner_up"] = {"kernel": kernel_label(t2)[1], "kernel_symbol": kernel_label(t2)[0], "launches_per_step": d2["n"],
                            "avg_launch_us": round(d2["ms"] / d2["n"] * 1e3, 2),
                            "share_of_serial_step": round(d2["ms"] / tot_ms, 4), "intensity_flop_per_byte": round(in2, 1),
                            "bound": "mfma" if in2 >= ridge else "hbm", "frac_mfma": round(tf2 / peak_tflops, 4), "frac_hbm": round(gb2 / PEAK_HBM_GBS, 4)}
        busy2, _, _ = pmc_mfma_busy(kernel_label(t2)[0], tag)  # (from the committed SQ pass, like the dominant kernel's)
        out["runner_up"]["mfma_busy"] = busy2
    out["share_of_serial_step"] = round(dom["ms"] / tot_ms, 4)
    if warm is not None:
        out["back_to_back_us"] = round(sum(p["ms"] for p in warm if p["tile"] == dom_tile) / dom["n"] * 1e3, 2)
    if frames_dev is not None:
        # the same timestamps with the parser in the loop, as in the timed region with one pipe (and as rocprofv3 sees the kernel in
        # profiles/*_kernel_stats*.csv, collected from `bench.py --pipes 1`): the parser's kernels run between two engine passes and
        # evict the weights from L2
        ms = n = 0
        for _ in range(iters):
            pipe.submit(frames_dev, True, engine=False, parser=True)
            pipe.collect()
            for q in pipe.eng.profile(batch, iters=1, in_sequence=True):
                if q["tile"] == dom_tile:
                    ms += q["ms"]
                    n += 1
        out["avg_launch_us_parser_in_loop"] = round(ms / n * 1e3, 2)
    return out


# ------------------------------------------------------------------------------------------------ clocks
class ClockSampler:
    """Shader clock / socket power of one GPU sampled from amdgpu's sysfs files by a side thread (every 20 ms) while a timed region runs -
    the counter behind every statement about sustained clocks: `sclk_mhz_mean / min / max` say at which clock
    the fractions of the NOMINAL peak (2.4 GHz) in the roofline objects were achieved.  Sources, first one that answers: hwmon
    freq1_input (Hz) and power1_average / power1_input (uW); pp_dpm_sclk (the starred level).  Nothing readable -> all null."""

    def __init__(self, device_index: int = 0, period_s: float = 0.02):
        import glob
        import threading
        self.period, self.samples, self.power = period_s, [], []
        self._stop = threading.Event()
        self._thread = None
        self.freq_file = self.power_file = self.dpm_file = None
        cards = sorted(p for p in glob.glob("/sys/class/drm/card[0-9]*") if os.path.exists(os.path.join(p, "device", "pp_dpm_sclk")))
        # the sysfs card of HIP device `device_index`: by PCI address (a box exposes ONE of its GPUs to the process, and card0 is rarely it)
        self.pci = self._pci_bus_id(device_index)
        dev = None
        if self.pci:
            for c in cards:
                if os.path.basename(os.path.realpath(os.path.join(c, "device"))).lower() == self.pci.lower():
                    dev = os.path.join(c, "device")
        elif device_index < len(cards) and device_index >= 0:
            dev = os.path.join(cards[device_index], "device")
        if dev:
            for h in sorted(glob.glob(os.path.join(dev, "hwmon", "hwmon*"))):
                f = os.path.join(h, "freq1_input")
                if os.path.exists(f) and self.freq_file is None:
                    self.freq_file = f
                for name in ("power1_average", "power1_input"):
                    f = os.path.join(h, name)
                    if os.path.exists(f) and self.power_file is None:
                        self.power_file = f
            self.dpm_file = os.path.join(dev, "pp_dpm_sclk")
        self.source = None

    @staticmethod
    def _pci_bus_id(device_index):
        """'0000:05:00.0' of a HIP device (hipDeviceGetPCIBusId through the runtime libhp_hip.so already loaded), or None."""
        import ctypes
        if device_index < 0:
            return None
        for name in ("libamdhip64.so", "libamdhip64.so.7", "libamdhip64.so.6"):
            try:
                hip = ctypes.CDLL(name)
                buf = ctypes.create_string_buffer(64)
                if hip.hipDeviceGetPCIBusId(buf, 64, int(device_index)) == 0:
                    return buf.value.decode().strip() or None
            except (OSError, AttributeError):
                continue
        return None

    def _read_mhz(self):
        if self.freq_file:
            try:
                v = int(open(self.freq_file).read().strip())
                if v > 0:
                    self.source = "hwmon freq1_input"
                    return v / 1e6
            except (OSError, ValueError):
                pass
        if self.dpm_file:
            try:
                for line in open(self.dpm_file):
                    if "*" in line:
                        self.source = "pp_dpm_sclk"
                        return float(line.split(":")[1].lower().replace("mhz", "").replace("*", "").strip())
            except (OSError, ValueError, IndexError):
                pass
        return None

    def _run(self):
        while not self._stop.is_set():
            v = self._read_mhz()
            if v is not None:
                self.samples.append(v)
            if self.power_file:
                try:
                    self.power.append(int(open(self.power_file).read().strip()) / 1e6)
                except (OSError, ValueError):
                    pass
            self._stop.wait(self.period)

    def __enter__(self):
        import threading
        self.samples, self.power = [], []
        self._stop.clear()
        self._thread = threading.Thread(target=self._run, daemon=True)
        self._thread.start()
        return self

    def __exit__(self, *exc):
        self._stop.set()
        self._thread.join()

    def summary(self):
        s, p = self.samples, self.power
        return {"sclk_mhz_mean": round(sum(s) / len(s), 1) if s else None, "sclk_mhz_min": round(min(s), 1) if s else None,
                "sclk_mhz_max": round(max(s), 1) if s else None, "samples": len(s), "source": self.source,
                "power_w_mean": round(sum(p) / len(p), 1) if p else None, "power_w_max": round(max(p), 1) if p else None,
                "nominal_peak_clock_mhz": 2400, "pci": self.pci}


LAST_OUTPUTS = {}  # workload key -> the humans (one structured array per frame) its timed path returned in its last step
DUMP_LIMIT_BYTES = 64 << 20
HUMAN_SLOTS = 128  # humans per frame the output buffer of every parser / hp_pipeline_* this bench creates holds (cap_per_frame)


def _humans_f32(h) -> np.ndarray:
    """[n, 73] float32 rows of one frame's humans: per body part (has_value, x, y, score) x 18, then the human's score."""
    out = np.zeros((len(h), 18 * 4 + 1), np.float32)
    for k, f in enumerate(("has_value", "x", "y", "score")):
        out[:, k:72:4] = h["parts"][f]
    out[:, 72] = h["score"]
    return out


def dump_outputs(out_dir, cfg, batch, rank):
    """--dump-outputs: what the headline's timed path returned in its last step - the humans of every frame of the batch, in the layout of
    the C ABI's output buffer: humans.npy [batch, HUMAN_SLOTS, 73], frame f's humans in its first humans_per_frame[f] rows, zeros after them
    (so the file's shape does not depend on how many humans a build finds) - and, since the
    synthetic weights give heat-maps without people, the conv stack's own outputs for the same frames (an Engine of the same model, weights
    and precision, run once after the timed steps).  float32 .npy files, <= 64 MB in all: a larger map is replaced by a fixed seeded sample
    of its elements (`<name>_sample.npy`)."""
    from hyperpose_amd.engine import Engine, Model
    os.makedirs(out_dir, exist_ok=True)
    last = LAST_OUTPUTS.get(cfg["key"]) or []
    slots = np.zeros((batch, max([HUMAN_SLOTS] + [len(h) for h in last]), 18 * 4 + 1), np.float32)
    for f, h in enumerate(last[:batch]):
        slots[f, :len(h)] = _humans_f32(h)
    np.save(os.path.join(out_dir, "humans_per_frame.npy"), np.array([len(h) for h in last[:batch]] + [0] * (batch - len(last)), np.float32))
    np.save(os.path.join(out_dir, "humans.npy"), slots)
    model = Model(cfg["arch"], cfg["w"], cfg["h"])
    eng = Engine.from_model(model, model.init_weights(cfg["seed"]), max_batch=batch, dtype=cfg["dtype"])
    per_frame = eng.inference(synth_frames(cfg, batch, rank))
    maps = {name: np.ascontiguousarray(np.stack([dict(f)[name] for f in per_frame]), np.float32) for name, _ in per_frame[0]}
    budget = DUMP_LIMIT_BYTES - (1 << 20)
    total = sum(a.nbytes for a in maps.values())
    rng = np.random.default_rng(20240)
    for name, a in sorted(maps.items()):
        if total <= budget:
            np.save(os.path.join(out_dir, f"dnn_{name}.npy"), a)
        else:
            k = int(a.size * budget / total)
            idx = np.sort(rng.choice(a.size, k, replace=False))
            np.save(os.path.join(out_dir, f"dnn_{name}_sample.npy"), a.reshape(-1)[idx])
    eng.close()


def measure(cfg, args, rank, world, dev, scaling, steps, warmup, headline, light=False):
    """Time one BASELINE configuration at one engine precision; returns the dict of its numbers (identical on every rank where it
    matters).  `light`: the end-to-end rate, the legs and the roofline only (no CPU baseline, no host-fed legs)."""
    import math

    import torch
    import torch.distributed as dist

    from hyperpose_amd import _lib
    from hyperpose_amd import dist as hd
    from hyperpose_amd.engine import Model

    batch, global_batch = rank_plan(cfg["batch"], scaling, rank, world)
    model = Model(cfg["arch"], cfg["w"], cfg["h"])
    # one-time weight broadcast from rank 0 over RCCL/xGMI (the only collective of the whole job)
    w_host = hd.broadcast_weights(model.init_weights(cfg["seed"]) if rank == 0 else None, model.n_weights, rank, world,
                                  device=hd.collective_device(dev))

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    coll = None
    if world > 1:
        coll = {"backend": hd.LAST_BROADCAST.get("backend"), "bcast_bytes": hd.LAST_BROADCAST.get("bytes"), "bcast_ms": hd.LAST_BROADCAST.get("ms"),
                "what": "one broadcast of the fp32 weight blob from rank 0 at start-up (outside the timed region); the steady state has no collective"}
    n_pipes = args.pipes if args.pipes > 0 else cfg["pipes"]
    res = {"workload": cfg["label"], "key": cfg["key"], "dtype": cfg["dtype"], "dtype_long": DTYPE_LONG[cfg["dtype"]],
           "frames_per_gpu_per_step": batch, "global_batch": global_batch, "scaling": scaling,
           "pipes_per_gpu": n_pipes, "gflop_per_frame": round(model.flops_per_frame / 1e9, 2)}
    if coll:
        res["collective"] = coll
    full = args.full
    resident = full or cfg["dtype"] == "f32s"  # (HP_DTYPE_F32S: the resident loop is the headline itself)
    if batch == 0:  # strong scaling with more ranks than frames: this rank idles but still takes part in the barriers
        pipes, frames_dev, maps = [], None, None
    elif not resident:  # a plain run: the host-fed headline alone
        pipes, frames_dev, maps = [], None, None
        frames = synth_frames(cfg, batch, rank)
    else:
        frames, maps = synth_inputs(cfg, batch, rank)
        frames_dev = _lib.DevBuf.from_numpy(frames)
        inj = [_lib.DevBuf.from_numpy(m) for m in maps]
        pipes = [Pipe(cfg, model, w_host, inj, batch) for _ in range(max(1, n_pipes))]
    sampler = None if (not full or args.no_clocks or rank != 0) else ClockSampler(dev.index or 0)

    def timed_region(run, active, min_s):
        """W warm-up steps + a 0.3 s ramp of the same loop (both untimed), then ONE timed region of R x K steps - R the smallest whole
        number that makes it last >= --min-seconds (from the ramp's own rate; the MAX over the ranks, so that every rank runs the same
        count) - bracketed by barrier + synchronize on both sides.  run(n): n more steps AND their results on the host (the region ends
        when the last human of the last batch is there)."""
        est = None
        if active:
            run(warmup)
            # the GPU's clocks take a few hundred ms of load to settle (100 steps right after a short warm-up measure ~12 % low): keep
            # the same loop running, untimed, until 0.3 s have passed since the warm-up ended
            torch.cuda.synchronize()
            t_ramp, n_ramp = time.perf_counter(), 0
            while time.perf_counter() - t_ramp < 0.3:
                n_ramp += run(max(1, n_pipes))
            torch.cuda.synchronize()
            est = (time.perf_counter() - t_ramp) / max(1, n_ramp)
        reps = max(1, math.ceil(min_s / (steps * est))) if (est and min_s > 0) else 1
        reps = int(round(hd.max_over_ranks(float(reps), world, device=hd.collective_device(dev))))
        n_timed = steps * reps
        barrier()
        if sampler:
            sampler.__enter__()
        t0 = time.perf_counter()
        if active:
            run(n_timed)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if sampler:
            sampler.__exit__()
        dt = hd.max_over_ranks(dt, world, device=hd.collective_device(dev))
        barrier()
        return dt, n_timed

    humans = [0]
    # the headline's region is exactly `steps` steps unless --min-seconds asks for more; every other region of --full lasts >= SECONDARY_MIN_S
    head_min_s = args.min_seconds or 0.0
    other_min_s = SECONDARY_MIN_S if args.min_seconds is None else args.min_seconds

    def timed(injected, min_s):
        def run(n):
            humans[0] += run_loop(pipes, frames_dev, n, injected)
            return n
        humans[0] = 0
        dt_, n_ = timed_region(run, bool(pipes), min_s)
        return dt_, humans[0], n_

    res["unit"], res["steps"] = "frames/s", steps
    peak = PEAKS[cfg["dtype"]]
    if resident:
        dt_res, n_humans, n_res = timed(True, head_min_s if (headline and cfg["dtype"] == "f32s") else other_min_s)
        if pipes:
            LAST_OUTPUTS[cfg["key"]] = pipes[(n_res - 1) % len(pipes)].last
        clocks_resident = sampler.summary() if sampler else None
        dt_dnn, n_dnn = None, 0
        if full and headline and not args.no_dnn_output:
            dt_dnn, _, n_dnn = timed(False, other_min_s)
        # host fall-backs / truncations over every step this rank ran (warm-up and both resident phases): frames a device decoder declined and
        # handed to the host statements (PoseProposal / PifPaf), batches with an overflowed PAF list
        parsed = sum(p.frames_parsed for p in pipes)
        res.update({"device_declined_frames": sum(p.declined_frames for p in pipes), "capacity_truncations": sum(p.capacity_truncations for p in pipes),
                    "frames_parsed_for_these_counts": parsed})
        res.update({"value_resident_injected": round(global_batch * n_res / dt_res, 1), "ms_per_step_resident_injected": round(dt_res / n_res * 1e3, 4),
                    "steps_timed_resident_injected": n_res, "humans_per_step_resident_injected": n_humans / max(1, n_res),
                    "what_resident_injected": "round 5's headline: u8 frames already resident in HBM, the full conv stack, the parser fed seeded synthetic "
                                              "heat-maps with several people per frame (injected; the network's random weights give maps without people), "
                                              "humans to pinned host memory",
                    "fps_dnn_output": round(global_batch * n_dnn / dt_dnn, 1) if dt_dnn else None})
        if clocks_resident:
            res["clocks_resident_injected"] = clocks_resident
    if full and rank == 0 and pipes and not args.no_roofline:
        # where the step's time goes: the parser alone (injected maps: GPU kernels + the host tail in collect) and the conv stack
        # alone, each through ONE pipe, next to the end-to-end step above (in which several pipes overlap them)
        p0 = pipes[0]

        def leg(eng_on, par_on, min_s=0.4, injected=True):
            """ms per step of ONE pipe running the given halves serially: 0.15 s ramp, then >= min_s timed (independent of --steps)."""
            t_r = time.perf_counter()
            while time.perf_counter() - t_r < 0.15:
                p0.submit(frames_dev, injected, engine=eng_on, parser=par_on)
                p0.collect()
            torch.cuda.synchronize()
            n, t0 = 0, time.perf_counter()
            while n < 4 or time.perf_counter() - t0 < min_s:
                p0.submit(frames_dev, injected, engine=eng_on, parser=par_on)
                p0.collect()
                n += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3

        db = p0.eng.device_bytes   # HBM one engine holds for this batch (activations with halos, weights in every packed form, fp32 outputs)
        res["engine_hbm_mb"] = {k: round(v / 2 ** 20, 1) for k, v in db.items()}
        res["engine_hbm_mb"]["all_pipes_total"] = round(db["total"] * len(pipes) / 2 ** 20, 1)
        res["parser_only_ms_per_step"] = round(leg(False, True), 4)
        res["engine_only_ms_per_step"] = round(leg(True, False), 4)
        res["parser_share_of_serial_step"] = round(res["parser_only_ms_per_step"] / (res["parser_only_ms_per_step"] + res["engine_only_ms_per_step"]), 4)
        if headline:  # the parser alone on the network's OWN maps (random weights: dense noise instead of a few people - the parser's worst case)
            res["parser_only_dnn_output_ms_per_step"] = round(leg(False, True, injected=False), 4)
        # one engine + parser pair, one batch in flight at a time: what a caller that does not pipeline batches gets - with the batch on one
        # stream (round 5's figure), and as two half-batches side by side (hp_engine_set_concurrency(2), HP_DTYPE_F32 engines: what the C++
        # mirror's synchronous tensorrt::inference uses)
        res["single_pipe_fps_one_stream"] = round(batch / (leg(True, True) * 1e-3), 1)
        res["single_pipe_fps"] = res["single_pipe_fps_one_stream"]
        if cfg["dtype"] == "f32" and batch >= 2:
            p0.eng.set_concurrency(2)
            res["engine_only_two_halves_ms_per_step"] = round(leg(True, False), 4)
            res["single_pipe_fps"] = round(batch / (leg(True, True) * 1e-3), 1)
            p0.eng.set_concurrency(1)
        pb = PARSER_BYTES[cfg["parser"]](cfg["h"], cfg["w"])
        gbs = batch * pb / (res["parser_only_ms_per_step"] * 1e-3) / 1e9
        res["parser_roofline"] = {"bound": "hbm", "achieved": round(gbs, 2), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 5),
                                  "bytes_per_frame": pb, "frames_per_s_parser_alone": round(batch / (res["parser_only_ms_per_step"] * 1e-3), 1),
                                  "what": "compulsory bytes (the network's output tensors read once, SURVEY.md 8d) x frames/s of the parser alone "
                                          "(one pipe, injected maps, GPU kernels + collect); latency-bound at these sizes, not bandwidth-bound"}
        del p0
    if full and rank == 0 and pipes:
        if not args.no_roofline:
            res["roofline"] = roofline(pipes[0], batch, cfg, frames_dev)
        if world == 1 and not args.no_cpu_baseline and not light:
            res["cpu_baseline"] = cpu_baseline(cfg, maps)
    # ---- `value`: SURVEY.md 8(d) / BASELINE.md 4.5 - the whole batch INCLUDING the H2D of its u8 frames and the D2H of its
    # humans, the parser on the network's OWN output: frames in pinned host memory -> ONE H2D copy per batch -> conv stack -> parser -> humans on
    # the host, through the stream operator's device pipeline (hp_pipeline_*) with the same pipes per GPU, on EVERY rank at once (each rank its own
    # pinned frames, all fed from the same host), under the same protocol as above (warm-up, ramp, R x K steps between barriers, MAX over the ranks).
    del pipes[:]
    if cfg["dtype"] == "f32s":  # (hp_pipeline_* refuses this opt-in type - its overflow guard never runs there: its value is the resident figure, and says so)
        res.update({"value": res["value_resident_injected"], "ms_per_step": res["ms_per_step_resident_injected"], "steps_timed": n_res, "timed_region_s": round(dt_res, 4),
                    "humans_per_step": n_humans / max(1, n_res), "what": res["what_resident_injected"] + " (no host-fed leg: hp_pipeline_* refuses HP_DTYPE_F32S)",
                    "conv_tflops_end_to_end": round(res["value_resident_injected"] * model.flops_per_frame / 1e12, 2),
                    "conv_frac_of_mfma_peak_end_to_end": round(res["value_resident_injected"] * model.flops_per_frame / 1e12 / peak / world, 4)})
        return res
    fed = HostFed(model, w_host, cfg, batch, n_pipes, (cfg["w"], cfg["h"]), False, frames_u8=frames) if batch else None

    def run_fed(n):
        fed.run(n)
        fed.drain()
        return n

    def run_fed_open(n): # (ramp / warm-up: no drain per call)
        fed.run(n)
        return n

    if fed:
        run_fed_open(max(2 * n_pipes, 4))
        fed.drain()
    dt, n_timed = timed_region(run_fed, bool(fed), head_min_s if headline else other_min_s)
    if sampler:
        res["clocks"] = sampler.summary()
    fps = global_batch * n_timed / dt
    res.update({"value": round(fps, 1), "steps_timed": n_timed, "timed_region_s": round(dt, 4), "ms_per_step": round(dt / n_timed * 1e3, 4),
                "humans_per_step": (fed.humans / max(1, n_timed + warmup)) if fed else 0.0,
                "what": f"network-sized {cfg['w']}x{cfg['h']} u8 BGR frames in pinned host memory -> ONE H2D copy per batch ({(fed.nbytes * batch if fed else 0) / 1e6:.2f} MB) -> "
                        "conv stack -> parser (the network's own heat-maps) -> humans on the host",
                "conv_tflops_end_to_end": round(fps * model.flops_per_frame / 1e12, 2),
                "conv_frac_of_mfma_peak_end_to_end": round(fps * model.flops_per_frame / 1e12 / peak / world, 4)})
    # (kept under its round-5 name too: tests and older readers)
    res["h2d_inclusive"] = {"value": res["value"], "unit": "frames/s", "steps": n_timed, "n_gpus": world, "what": res["what"]}
    if fed:
        LAST_OUTPUTS[cfg["key"]] = fed.last
        fed.close()
    if full and rank == 0 and headline and world == 1 and not light:
        if not args.no_from_host:
            res["from_host"] = from_host(model, w_host, cfg, batch, n_pipes)
        # the drop-in operator API itself, one batch in flight (VERDICT r5 missing #3): the C++ mirror's engine.inference + parser.process loop
        if not args.no_operator_api:
            res["operator_api"] = operator_api(cfg, batch)
    return res


# ------------------------------------------------------------------------------------------------ the ONE line
LINE_LIMIT = 3800  # 4096 is the judge's bound; the driver's parser takes the last stdout line; 13 KB parsed in round 3, 21 KB did not in round 4: stay far below


def _short(s, n):
    s = str(s)
    return s if len(s) <= n else s[: n - 1] + "~"


def compact_roofline(r):
    """The roofline object of the printed line: the contract's keys + both fractions + the kernel's symbol + what the committed
    rocprofv3 trace says about the same kernel (source file, its average, the fraction recomputed with it)."""
    if not r:
        return None
    cp = r.get("committed_profile") or {}
    frac_key = "frac_mfma" if r["bound"] == "mfma" else "frac_hbm"
    return {"bound": r["bound"], "achieved": r["achieved"], "peak": r["peak"], "unit": r["unit"], "frac": r["frac"], "traffic": r["traffic"],
            "mfma_busy": r.get("mfma_busy"), "mfma_busy_source": r.get("mfma_busy_source"),
            "frac_mfma": r["frac_mfma"], "frac_hbm": r["frac_hbm"], "kernel": _short(r.get("kernel_symbol") or r["kernel"], 80),
            "launches_per_step": r["launches_per_step"], "avg_launch_us": r["avg_launch_us"],
            "flops_per_launch": r["flops_per_launch"], "algorithmic_bytes_per_launch": r["algorithmic_bytes_per_launch"],
            "all_mfma_convs_frac": r["all_mfma_convs"]["frac"],
            **({"frac_mfma_issued": r["frac_mfma_issued"], "note": "Winograd F(2x2,3x3): frac = algorithmic (direct-form) flops / time / peak; frac_mfma_issued = the 16/36 of them the pipe executes"}
               if "frac_mfma_issued" in r else {}),
            "committed_profile": {"source": cp.get("source"), "avg_launch_us": cp.get("avg_launch_us"), "frac": cp.get(frac_key)},
            # the kernel with the second-largest share of the step, in four numbers (the rest: the detail file)
            **({"runner_up": {"kernel": _short((r["runner_up"].get("kernel_symbol") or ""), 40), "share": r["runner_up"].get("share_of_serial_step"),
                              "frac": r["runner_up"].get("frac_mfma" if r["runner_up"].get("bound") == "mfma" else "frac_hbm"),
                              "mfma_busy": r["runner_up"].get("mfma_busy")}} if r.get("runner_up") else {})}


def compact_line(detail):
    """The ONE JSON line rank 0 prints: the contract's keys, the headline's roofline and cpu_baseline, one small object per other
    workload - everything else lives in the detail file it names.  Pure function of the detail record (tests/test_bench_labels.py)."""
    head, a = detail["headline"], detail["args"]
    cfg_i = head["key"]
    out = {
        "metric": detail["metric"], "value": head["value"], "unit": "frames/s", "n_gpus": detail["n_gpus"], "steps": a["steps"], "warmup": a["warmup"],
        "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": head["scaling"], "vs_baseline": None,
        "dtype": DTYPE_LABEL[head["dtype"]], "data": "synthetic",
        "config": {"workload": _short(head["workload"] + " per GPU; frames from pinned host memory (one H2D per batch), parser on the network's own maps, humans to the host", 210),
                   "key": cfg_i, "engine": _short(head["dtype_long"], 100),
                   "global_batch": head["global_batch"], "frames_per_gpu_per_step": head["frames_per_gpu_per_step"],
                   "parallelism": f"frame-sharded x{detail['n_gpus']}, no steady-state collective", "pipes_per_gpu": head["pipes_per_gpu"],
                   "parser_input": "the network's own heat-maps", "gflop_per_frame": head["gflop_per_frame"]},
        "steps_timed": head["steps_timed"], "timed_region_s": head["timed_region_s"],
        # round 5's headline (frames resident in HBM, parser on injected synthetic maps with people) and the same with the network's own maps
        "value_resident_injected": head.get("value_resident_injected"), "fps_dnn_output": head.get("fps_dnn_output"),
        "value_h2d_inclusive": (head.get("h2d_inclusive") or {}).get("value"),
        # ONE batch in flight: one engine + parser pair driven through the C ABI, and the reference's operator-API loop through the C++ mirror
        "single_pipe_fps": head.get("single_pipe_fps"), "operator_api_fps": (head.get("operator_api") or {}).get("operator_api_fps"),
        "conv_tflops_end_to_end": head["conv_tflops_end_to_end"],
        "device_declined_frames": head.get("device_declined_frames"), "capacity_truncations": head.get("capacity_truncations"),
        "roofline": compact_roofline(head.get("roofline")),
    }
    cb = head.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {"value": cb["value"], "unit": "frames/s (parser only)", "cores": cb["cores"], "host_cores": cb["host_cores"],
                               "kind": cb["kind"], "sample": _short(cb["sample"], 110)}
    ck = head.get("clocks")
    if ck:
        out["clocks"] = {k: ck[k] for k in ("sclk_mhz_mean", "sclk_mhz_min", "power_w_mean")}
    if detail.get("collective_backend"):
        out["collective_backend"] = detail["collective_backend"]
    wl = {}
    for key, w in detail.get("workloads", {}).items():
        r = w.get("roofline") or {}
        wl[key] = {"value": w["value"], "resident": w.get("value_resident_injected"), "bound": r.get("bound"), "frac": r.get("frac")}  # (ms_per_step etc.: the detail file)
        if "frac_mfma_issued" in r:  # a Winograd kernel dominates: `frac` counts direct-form flops (may pass 1), `issued` what the pipe executes
            wl[key]["issued"] = r["frac_mfma_issued"]
    if wl:
        out["workloads"] = wl
        # host fall-backs / truncated lists over ALL workloads of the run (per workload: the detail file)
        out["device_declined_frames_all"] = sum(w.get("device_declined_frames") or 0 for w in [head] + list(detail["workloads"].values()))
        out["capacity_truncations_all"] = sum(w.get("capacity_truncations") or 0 for w in [head] + list(detail["workloads"].values()))
    if cfg_i == "configs[1]/f32":
        # the two other engines of the same workload: kHALF (fused fp16, the optional fast mode) and the opt-in HP_DTYPE_F32S
        # (fp32 storage / accumulation, products as three exact fp16 x fp16 MFMAs: its peak is 2500 / 3 TFLOP/s of fp32-equivalent work)
        for tag, key in (("khalf", "configs[1]/f16"), ("f32_split", "configs[1]/f32s")):
            w = detail.get("workloads", {}).get(key)
            if w:
                out["value_" + tag] = w["value"]
                r = compact_roofline(w.get("roofline"))
                if r:
                    for k in ("flops_per_launch", "algorithmic_bytes_per_launch", "all_mfma_convs_frac", "traffic", "mfma_busy_source", "note", "frac_mfma", "frac_hbm", "runner_up"):
                        r.pop(k, None)
                out["roofline_" + tag] = r
    out["detail"] = detail.get("detail_file")
    line = json.dumps(out, separators=(",", ":"))
    # never let the line outgrow the driver's parser: drop the optional parts, largest first
    for k in ("roofline_f32_split", "roofline_khalf", "workloads", "clocks"):
        if len(line) <= LINE_LIMIT:
            break
        out.pop(k, None)
        out["dropped_for_size"] = out.get("dropped_for_size", []) + [k]
        line = json.dumps(out, separators=(",", ":"))
    return line


def parse_extra(extra, world, headline_key):
    """[(index, dtype)] of the workloads measured besides the headline.  Default at N = 1: configs[1] at the other precision, then every
    other BASELINE configuration at both precisions; at N > 1: configs[3], configs[4] (the frame-sharded ones) at the headline's precision,
    strong-scaled."""
    out = []
    for tok in [t.strip() for t in extra.split(",") if t.strip()]:
        i, _, d = tok.partition("/")
        if int(i) == 5:
            i, d = 1, "f32"
        for dd in ([d] if d else ["f32", "f16"]):
            if int(i) in CONFIGS and dd in DTYPE_LONG and f"configs[{int(i)}]/{dd}" != headline_key and (int(i), dd) not in out:
                out.append((int(i), dd))
    return out


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(respawn(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    import torch.distributed as dist

    from hyperpose_amd import _lib
    from hyperpose_amd import dist as hd

    # one rank per GPU.  HP_BENCH_SHARE_DEVICES=1 (tests of the multi-rank path on a box with fewer GPUs than ranks): ranks wrap around the
    # visible devices - RCCL refuses two ranks on one GPU, the ranks then agree on gloo for the start-up broadcast (hyperpose_amd/dist.py)
    n_dev = torch.cuda.device_count()
    if local_rank >= n_dev and n_dev > 0 and os.environ.get("HP_BENCH_SHARE_DEVICES"):
        local_rank %= n_dev
    torch.cuda.set_device(local_rank)
    _lib.init(local_rank)
    dev = torch.device("cuda", local_rank)
    backend = None
    if world > 1:
        backend = hd.init_for_gpu(dev)  # RCCL, or - agreed by all ranks - gloo if it cannot be brought up (the hot path has no collective)

    cfg = config(args.config, args.dtype)
    steps = args.steps if args.steps is not None else cfg["steps"]
    head = measure(cfg, args, rank, world, dev, args.scaling, steps, args.warmup, True)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, cfg, head["frames_per_gpu_per_step"], rank)
    detail = {
        "metric": "end-to-end FPS (preproc+DNN+PAF parse) @ 368x432" if args.config in (0, 1) else f"end-to-end FPS (preproc+DNN+parse), {cfg['label']}",
        "n_gpus": world, "args": {"steps": steps, "warmup": args.warmup, "config": args.config, "dtype": args.dtype, "scaling": args.scaling,
                                  "min_seconds": args.min_seconds, "pipes": args.pipes},
        "collective_backend": backend, "headline": head, "workloads": {},
    }
    extra = args.extra
    if extra is None:
        if not args.full or args.config != 1:
            extra = ""
        elif world == 1:
            other = "f16" if args.dtype == "f32" else "f32"
            extra = f"1/{other},1/f32s,0/{args.dtype},2/{args.dtype},3/{args.dtype},4/{args.dtype},0/{other},2/{other},3/{other},4/{other}"
        else:
            extra = f"3/{args.dtype},4/{args.dtype}"
    for k, dt_ in parse_extra(extra, world, cfg["key"]):
        c = config(k, dt_)
        scal = "strong" if world > 1 else "weak"
        # configs[1] at the other precision keeps its CPU-free secondary legs; the others run the light form
        r = measure(c, args, rank, world, dev, scal, c["steps"], max(2, min(args.warmup, c["steps"] // 4)), False, light=True)
        r["n_gpus"] = world
        detail["workloads"][c["key"]] = r
    if rank == 0 and not (args.full or args.detail):
        detail["detail_file"] = None  # a plain run writes no detail record
        print(compact_line(detail), flush=True)
    elif rank == 0:
        paths = [args.detail] if args.detail else [os.path.join(ROOT, "bench_detail.json")]
        if not args.detail and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
            paths.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
        detail["detail_file"] = os.path.relpath(paths[0], ROOT) if paths[0].startswith(ROOT) else paths[0]
        for p in paths:
            try:
                with open(p, "w") as f:
                    json.dump(detail, f, indent=1)
            except OSError as e:
                print(f"bench.py: could not write {p}: {e}", file=sys.stderr)
        print(compact_line(detail), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
