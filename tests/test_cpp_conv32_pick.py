"""The fp32 dense-convolution picker (csrc/conv32_pick.hpp) in a stand-alone host program: over a grid of forms, kernel sizes, channels, maps,
batches, switches and views it reproduces tests/golden/conv32_pick.txt - kernel, template arguments, grid, block, LDS bytes, kernel arguments and
tile code as the launchers' own arithmetic answered before the picker replaced it, and the weight forms the engine's lowerings gave a layer - and
every choice is a compiled instance whose grid covers the layer (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "conv32_pick.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "conv32_pick.bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv32_pick.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_picker_reproduces_the_recorded_choices_and_is_self_consistent():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           SRC, "-o", BIN])
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    assert tag == "OK" and int(checks) > 5000
