"""CPU: the HP_DTYPE_I8 additions to the C ABI and the C++ mirror - the ctypes mirror of hp_engine_desc has the C layout (a g++ probe of
include/hp_hip.h), and a program using data_type::kINT8 and tensorrt::calibrate() compiles against the mirror headers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import test_engine_int8_gpu as int8_gpu
from hyperpose_amd import engine as E
from oracle import ref_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_engine_desc_layout_matches_the_header(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "hp_hip.h"\n'
                   'int main() { std::printf("%zu %zu %zu %d\\n", sizeof(hp_engine_desc), offsetof(hp_engine_desc, int8_scales), '
                   'offsetof(hp_engine_desc, dtype), (int)HP_DTYPE_I8); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, off_scales, off_dtype, i8 = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert C.sizeof(E.EngineDesc) == size
    assert E.EngineDesc.int8_scales.offset == off_scales
    assert E.EngineDesc.dtype.offset == off_dtype
    assert E.DTYPE_I8 == i8 == 3
    assert E._DTYPES["i8"] == E.DTYPE_I8


@pytest.mark.parametrize("case", int8_gpu.SIGNED_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_signed_int8_cases_reach_sign_ties_and_clamps(case):
    """The inputs of test_engine_int8_gpu.py::test_int8_layer_on_signed_tying_saturating_inputs, evaluated by the oracle: under the
    hand-set power-of-two scale they hold the negative, saturating and tying values the GPU test is there for (and under the calibrated
    scale they do not, which is why the calibrated cases cannot see those paths)."""
    net, t0, _, _, fr, calib = int8_gpu.signed_case(case)
    outs = [int8_gpu.Out("x", t0, 0, case["cin"])]
    tensors = ref_net.run(net.layers[:1], outs, net.blob(), frames_u8=fr, match_fp16=True, return_tensors=True)[1]
    ctens = ref_net.run(net.layers[:1], outs, net.blob(), frames_u8=calib, match_fp16=True, return_tensors=True)[1]
    s_cal = np.float32(np.abs(ctens[t0]).max()) / np.float32(127)
    shares = int8_gpu.assert_input_shares(tensors[t0], int8_gpu.dyadic_scale(s_cal))
    assert shares["ties_even_floor"] >= 0.003          # rint differs from round-half-up / half-away on these
    v = tensors[t0].astype(np.float32) * (np.float32(1) / s_cal)
    assert (np.abs(v) >= 127.5).mean() < 1e-4 and (np.abs(v - np.floor(v) - 0.5) == 0).mean() < 1e-3


def test_mirror_int8_program_compiles(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "operator_api_int8.cpp")
    out = tmp_path / "operator_api_int8.o"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(out)])
    assert out.exists()
