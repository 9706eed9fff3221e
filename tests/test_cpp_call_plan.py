"""The engine's call plan (csrc/call_plan.hpp: what hp_engine_infer_u8 / hp_engine_infer_f32 decide between their arguments and their launches) in a
stand-alone host program: every combination of max_batch, n, concurrency, halves_ok, ensemble, captured graphs, host / device and entry is held
to a restatement of the rules infer_common and hp_engine::enqueue had before the header - refusal, image count, ranges and their streams,
stage and merge inside or around, the address the network reads, the uploads, the graph keys - and a literal table to the cases one checks by
hand (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "call_plan.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "call_plan.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_call_plan_against_the_parent_rules():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    # max_batch 1, 2, 3, 4, 8 with n = 0 .. max_batch + 1: 3 + 4 + 5 + 6 + 10 = 28 (max_batch, n) pairs x 64 settings = 1792 combinations, one
    # check of the refusal each; a plan takes 7 checks and 3 per range.  By the rules: the ensemble refuses every f32 call and every 2n > max_batch
    combos = sum(mb + 2 for mb in (1, 2, 3, 4, 8)) * 64
    plans = 0
    for mb in (1, 2, 3, 4, 8):
        for n in range(1, mb + 1):
            plans += 32 + 16 * (2 * n <= mb)  # ensemble off: 32 settings; on: the 16 u8 ones, when 2n fits
    assert f"plans {plans}\n" in out.stdout
    assert tag == "OK" and int(checks) >= combos + plans * 10
