"""CPU: the host side of hyperpose_amd/csrc/mapview.hpp (index plane, taps, pixel index, palettes, host painter) as a stand-alone program built with
g++ -fsanitize=address,undefined, on frames, maps and tables allocated with no slack (tests/cpp/mapview_rules.cpp): a read or a write outside one of
them, or an overflow in the integer rules, aborts the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "mapview_rules.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "mapview_rules.bin")


def test_mapview_rules_stay_inside_their_buffers_under_sanitizers():
    # the sanitizers' runtimes are linked statically: the program needs nothing of its environment to start
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-4000:]
    # 4 sweeps x 10 layouts x 8 orientations x 5 rois x the modes the maps allow (MAX and FIELD; the two-channel maps of three sweeps: both)
    assert out.stdout.split()[-2:] == ["OK", str(4 * 10 * 8 * 5 * 2)]
