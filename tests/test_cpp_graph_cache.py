"""The engine's cache of captured-graph executables (csrc/graph_cache.hpp: what run_call, drop_graphs and the engine's destructor use) in
a stand-alone host program with fake executables and a ledger (created / in flight on stream k / destroyed): no executable of a call is
destroyed before the call launched it, none while a launch may be in flight on any stream, each exactly once, never more than 64 entries after
a call, and a call whose keys all hit neither evicts nor synchronises.  The program also drives the order the engine had before the header
through the same ledger, which must report the launch of a destroyed executable (CPU; no library, no device code)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "graph_cache.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "graph_cache.bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_graph_cache_lifetimes_and_the_parent_order():
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", SRC, "-o", BIN])
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, f"exit {out.returncode}\n" + out.stdout[-2000:] + out.stderr[-2000:]
    assert "parent order: launch of a destroyed executable at the call on distinct pointer 33" in out.stdout
    tag, checks = out.stdout.split()[-2:]
    # 6 pools x 2 concurrencies x 4 seeds x 600 calls, at least 4 checks per call (bound, entries == live executables, hit or eviction rule,
    # the handle launched is the live one), and 6 at the end of each run: 57 888; the sequences at the bound and the checker's own add ~600.
    # Every run now exists twice - plain device batches, and mixed with host batches and the ensemble (keys from csrc/call_plan.hpp)
    assert tag == "OK" and int(checks) >= 2 * 57_888
