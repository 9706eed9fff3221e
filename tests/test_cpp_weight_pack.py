"""The engine's weight layouts (csrc/weight_pack.hpp) in a stand-alone host program: every source element sits where the layout's definition
puts it and everything else is zero - fp16 fragments, the fused head's second layer, the first convolution's padded rows, int8 quantisation and
reorder (CPU; the program needs neither the library nor device code, only the host side of the project's compiler for the fp16 conversions)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "weight_pack.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "weight_pack.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_every_weight_layout_places_its_source_and_nothing_else():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    assert tag == "OK" and int(checks) > 300000
