"""The engine's call plan with the scale ensemble (csrc/call_plan.hpp, call_settings::scales) in a stand-alone host program: every combination
of max_batch, n, K, flip, concurrency, halves_ok, captured graphs, host / device and entry is held to the rules include/hp_hip.h states - the
refusals in their order, (flip ? 2 : 1) * K * n images covering exactly the ranges, stage and merge inside or around, the uploads, keys that
differ across (flip, K) - and with K == 1 to the plan of a call_settings that does not name the field (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "call_plan_scales.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "call_plan_scales.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_call_plan_with_scales_against_the_rules():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    # the plans the rules admit: off (K = 1, no flip) 32 settings per (max_batch, n); under an ensemble the 16 u8 settings when the images fit
    plans = 0
    for mb in (1, 2, 3, 4, 8, 12):
        for n in range(1, mb + 1):
            for K in range(1, 5):
                plans += 32 if K == 1 else 16 * (K * n <= mb)   # no flip
                plans += 16 * (2 * K * n <= mb)                 # flip
    assert f"plans {plans}\n" in out.stdout
    combos = sum(mb + 2 for mb in (1, 2, 3, 4, 8, 12)) * 64 * 4
    assert tag == "OK" and int(checks) >= combos + plans * 8
