"""The HP_*_DBG block-timeline text (csrc/engine_timeline.cpp) in a stand-alone host program: for one synthetic stamp buffer per timeline
kind, an all-zero buffer per kind, conv32_kernel's residency records (1 block; 4096 blocks on 3 XCDs with late starters; equal durations) and
the block spans of 0, 1 and 1024 blocks it prints tests/golden/engine_timelines.txt byte for byte - the text the same code printed while it
was part of engine.cpp (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "engine_timeline.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "engine_timeline.bin")
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_timelines.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_timeline_text_is_the_recorded_text():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           SRC, "-o", BIN])
    out = subprocess.run([BIN, GOLDEN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, cases, size = out.stdout.split()[-3:]
    assert tag == "OK" and int(cases) == 23 and int(size) == os.path.getsize(GOLDEN)
