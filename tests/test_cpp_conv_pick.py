"""The dense-convolution picker (csrc/conv_pick.hpp) in a stand-alone host program: over a grid of kernels, channels, maps, batches, strides,
slices and both weight layouts it reproduces tests/golden/conv_pick.txt - weight layout, tile code, split-K factor and scratch bytes as the
four separate cascades it replaced answered - and every choice satisfies its own form's precondition (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "conv_pick.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "conv_pick.bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_pick.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_picker_reproduces_the_recorded_choices_and_is_self_consistent():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           SRC, "-o", BIN])
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    assert tag == "OK" and int(checks) > 10000
