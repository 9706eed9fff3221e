"""CPU: the YUV front-end's compile unit, disassembled for gfx950 with the flags hyperpose_amd/build.py gives it, uses no scratch memory,
writes nothing through the scalar unit and holds no packed fp32 FMA (the project keeps those out of units whose fp32 arithmetic runs next
to the engines' kernels: -fno-slp-vectorize).  Prints the register counts DESIGN.md quotes."""
import os
import re
import subprocess

from hyperpose_amd import build as hb


def test_resize_yuv_unit_is_clean(tmp_path):
    extra = dict(hb.UNITS)["resize_yuv.hip"]
    assert "-fno-slp-vectorize" in extra and "-ffp-contract=off" in extra
    asm = str(tmp_path / "resize_yuv.s")
    subprocess.check_call([hb.HIPCC, "-x", "hip", *hb.COMMON, *extra, "--cuda-device-only", "-S", os.path.join(hb.CSRC, "resize_yuv.hip"), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    assert "resize_yuv420_kernel" in text
    code = [ln.split(";")[0].strip() for ln in text.splitlines()]
    code = [ln for ln in code if ln and not ln.startswith(".")]
    assert not [ln for ln in code if re.match(r"(scratch_|buffer_)\w+", ln)], "scratch / buffer instructions"
    # scalar-unit memory writes, atomics and cache write-backs: every mnemonic that starts with s_ and names one of them
    assert not [ln for ln in code if re.match(r"s_\w*(store|atomic|dcache_wb|dcache_discard)", ln)], "scalar memory writes"
    assert not [ln for ln in code if ln.startswith("v_pk_fma_f32")], "packed fp32 FMA"
    meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", text)}
    print("resize_yuv420_kernel:", meta)
    assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0
    assert meta["vgpr_count"] <= 64  # 256-thread blocks at full occupancy
