"""CPU: the HP_DTYPE_I8 additions to the C ABI and the C++ mirror - the ctypes mirror of hp_engine_desc has the C layout (a g++ probe of
include/hp_hip.h), and a program using data_type::kINT8 and tensorrt::calibrate() compiles against the mirror headers."""
import ctypes as C
import os
import subprocess

from hyperpose_amd import engine as E

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


def test_mirror_int8_program_compiles(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "operator_api_int8.cpp")
    out = tmp_path / "operator_api_int8.o"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", str(out)])
    assert out.exists()
