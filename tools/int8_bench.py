"""kINT8 against kHALF and kHALF's per-layer schedule (HP_NO_FUSE=1) on BASELINE.json configs[0..4], frames resident on the device.

One call measures, alternating the three engines round by round: frames/s of the conv stack (engine only, graph replay, frames already in
HBM) for every configuration, and the in-sequence per-layer tables (hp_engine_profile_sequence) of configs[2] and configs[3].  Writes
profiles/int8_bench.json and profiles/int8_layer_times_config{2,3}.txt, and prints the 7 x 7 gate of configs[2]: every 7 x 7 layer's time
on the int8 kernel against the same layer on kHALF's conv_direct_kernel.

    python tools/int8_bench.py [--rounds 3] [--configs 0 1 2 3 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hyperpose_amd import _lib  # noqa: E402
from hyperpose_amd import engine as E  # noqa: E402

# BASELINE.json configs (bench.py CONFIGS): arch, network width, height, batch
CONFIGS = {0: ("lw_openpose_vggtiny", 432, 368, 1), 1: ("lw_openpose_mobilenet", 432, 368, 8), 2: ("openpose_vgg19", 768, 432, 16),
           3: ("pose_proposal_resnet50", 384, 384, 32), 4: ("pifpaf_resnet50", 385, 385, 64)}
STEPS = {0: 200, 1: 100, 2: 10, 3: 30, 4: 10}


def engines(arch, w, h, batch):
    m = E.Model(arch, w, h)
    wts = m.init_weights(20240)
    i8 = E.Engine.from_model(m, wts, max_batch=batch, dtype="i8")
    i8.calibrate(np.random.default_rng(7).integers(0, 256, (max(2, batch), h, w, 3), dtype=np.uint8))
    f16 = E.Engine.from_model(m, wts, max_batch=batch, dtype="f16")
    os.environ["HP_NO_FUSE"] = "1"
    try:
        f16l = E.Engine.from_model(m, wts, max_batch=batch, dtype="f16")
    finally:
        del os.environ["HP_NO_FUSE"]
    return m, {"kINT8": i8, "kHALF": f16, "kHALF_per_layer": f16l}


def fps(eng, dev, batch, steps):
    eng.enqueue_u8(dev.ptr.value, batch)
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.enqueue_u8(dev.ptr.value, batch)
    eng.synchronize()
    return batch * steps / (time.perf_counter() - t0)


def table(m, engs, batch, iters=5):
    prof = {k: {q["layer"]: q for q in e.profile(batch, iters, in_sequence=True)} for k, e in engs.items()}
    lines = [f"# per-layer device time (ms, in sequence, batch {batch}); tile codes: 8900000 + K conv_i8_direct_kernel, 8BBBKKK conv_i8_kernel",
             f"{'layer':>5} {'op':>3} {'geometry':>22} | {'kINT8 ms':>9} {'tile':>8} | {'kHALF/layer ms':>14} {'tile':>8} | {'kHALF ms':>9} {'tile':>8}"]
    for i, L in enumerate(m.layers):
        geo = f"{L.cin}->{L.cout} {L.kh}x{L.kw} s{L.stride} d{L.dil}"
        cols = []
        for k in ("kINT8", "kHALF_per_layer", "kHALF"):
            q = prof[k].get(i)
            cols.append(f"{q['ms']:9.4f} {q['tile']:8d}" if q else f"{'(fused)':>9} {'':>8}")
        lines.append(f"{i:5d} {L.op:3d} {geo:>22} | {cols[0]} | {cols[1]:>23} | {cols[2]}")
    tot = {k: sum(q["ms"] for q in prof[k].values()) for k in prof}
    lines.append("total ms: " + ", ".join(f"{k} {v:.3f}" for k, v in tot.items()))
    return prof, "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--configs", type=int, nargs="+", default=[0, 1, 2, 3, 4])
    a = ap.parse_args()
    _lib.init(0)
    out = {"unit": "frames/s, conv stack only, frames resident, graph replay; median of rounds, the three engines alternating", "configs": {}}
    for ci in a.configs:
        arch, w, h, batch = CONFIGS[ci]
        m, engs = engines(arch, w, h, batch)
        frames = np.random.default_rng(ci).integers(0, 256, (batch, h, w, 3), dtype=np.uint8)
        dev = _lib.DevBuf.from_numpy(frames)
        runs = {k: [] for k in engs}
        for _ in range(a.rounds):
            for k, e in engs.items():
                runs[k].append(fps(e, dev, batch, STEPS[ci]))
        scales = engs["kINT8"].int8_scales
        flops = {i: 2.0 * L.cout * L.kh * L.kw * L.cin for i, L in enumerate(m.layers) if L.op == E.OP_CONV}
        prof = {q["layer"]: q for q in engs["kINT8"].profile(batch, 1)}
        f_all = sum(prof[i]["flops"] for i in flops if i in prof)
        f_i8 = sum(prof[i]["flops"] for i in flops if i in prof and scales[i] > 0)
        res = {k: float(np.median(v)) for k, v in runs.items()}
        res.update(arch=arch, size=f"{w}x{h}", batch=batch, int8_layers=int((scales > 0).sum()), conv_layers=len(flops),
                   int8_flop_share=f_i8 / f_all if f_all else 0.0, rounds={k: [round(x, 1) for x in v] for k, v in runs.items()})
        out["configs"][f"configs[{ci}]"] = res
        print(json.dumps({f"configs[{ci}]": res}), flush=True)
        if ci in (2, 3):
            prof_t, txt = table(m, engs, batch)
            with open(os.path.join(ROOT, "profiles", f"int8_layer_times_config{ci}.txt"), "w") as f:
                f.write(f"# configs[{ci}] {arch} batch {batch} @ {h}x{w}\n" + txt)
            if ci == 2:
                gate = []
                for i, L in enumerate(m.layers):
                    if L.op == E.OP_CONV and L.kh == 7 and i in prof_t["kINT8"] and i in prof_t["kHALF"]:
                        gate.append(dict(layer=i, cin=L.cin, cout=L.cout, int8_ms=prof_t["kINT8"][i]["ms"], int8_tile=prof_t["kINT8"][i]["tile"],
                                         khalf_ms=prof_t["kHALF"][i]["ms"], khalf_tile=prof_t["kHALF"][i]["tile"]))
                out["gate_7x7_config2"] = gate
                for g in gate:
                    print(f"7x7 gate layer {g['layer']} {g['cin']}->{g['cout']}: int8 {g['int8_ms'] * 1e3:.1f} us (tile {g['int8_tile']}) vs kHALF "
                          f"{g['khalf_ms'] * 1e3:.1f} us (tile {g['khalf_tile']})", flush=True)
        for e in engs.values():
            e.close()
        dev.free()
        with open(os.path.join(ROOT, "profiles", "int8_bench.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
