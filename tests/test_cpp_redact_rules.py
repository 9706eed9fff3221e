"""CPU: the host side of hyperpose_amd/csrc/redact.hpp (region list + host painter) as a stand-alone program built with
g++ -fsanitize=address,undefined, on planes allocated with no slack (tests/cpp/redact_rules.cpp): a read or a write outside a plane, or an
overflow in the integer rules, aborts the program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "redact_rules.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "redact_rules.bin")


def test_redact_rules_stay_inside_their_planes_under_sanitizers():
    # the sanitizers' runtimes are linked statically: the program needs nothing of its environment to start
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
                           "-static-libubsan", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-4000:]
    # regions: 2 margins x (4 head discs + 5 body rectangles and 4 discs) + 5 at the limits = 31
    # 2 sizes x 10 layouts x (31 regions one at a time + their union) x 2 effects x 2 cells
    assert out.stdout.split()[-2:] == ["OK", str(2 * 10 * 32 * 4)]
