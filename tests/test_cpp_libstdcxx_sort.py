"""The one restatement of libstdc++'s std::sort (csrc/libstdcxx_sort.hpp) that the three parsers call on the device, in a stand-alone
host program against the real std::sort: index arrays with `>` and `<` on the keys, 24-byte boxes sorted in place (the PoseProposal NMS),
mass ties, random floats, monotone and organ-pipe runs, and McIlroy-adversary sequences that run the heap-sort fall-back (CPU; no
library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "libstdcxx_sort.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "libstdcxx_sort.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_restated_sort_leaves_what_std_sort_leaves():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    tag, checks = out.stdout.split()[-2:]
    # 12 sizes x (40 random + 4 fixed) + 10 adversary sequences, three sorts each, two checks per sort and a third where used_heap is set
    assert tag == "OK" and int(checks) >= 3000
