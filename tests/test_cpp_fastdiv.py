"""csrc/fastdiv.hpp (division by a layer's invariant divisors as multiply-high, add, shift) in a stand-alone host program: for every divisor
an fp32 engine of the five BASELINE networks forms, and for 1, 2, 3, 7, 16, 17, 54, 2 484, 2^16 - 1, 2^16 + 1 and the range's ends, quotient and
remainder equal `/` and `%` for every numerator below 2^24, a stride through the rest of the stated range [0, 2^31) and its end; and the
kernels' pixel -> (image, row) -> view index equals the carry loop it replaced on maps 1 .. 40 pixels wide (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fastdiv.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "fastdiv.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_fastdiv_is_exact_over_its_stated_range():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O2", "-Wall", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    assert tag == "OK" and int(checks) > 50 * (1 << 24)
