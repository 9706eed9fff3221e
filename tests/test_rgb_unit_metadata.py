"""CPU: the unit that holds the hp_rgb_image resize kernels (resize_rgb.hip), compiled to assembly for gfx950 with the flags hyperpose_amd/build.py
gives it.  Only the kernels' metadata is read: no scratch memory, no spilled registers, at most 64 VGPRs (256-thread blocks at full occupancy), for
every kernel of the unit - per Taps type both thread maps of the per-frame kernel and the many-regions kernel.  Prints the register counts."""
import os
import re
import subprocess

from hyperpose_amd import build as hb

UNIT = "resize_rgb.hip"
TAPS = ["rgb", "rgb32"]  # byte loads for every layout; one 32-bit load per tap for the 4-byte layouts


def test_resize_rgb_unit_metadata(tmp_path):
    extra = dict(hb.UNITS)[UNIT]
    assert "-fno-slp-vectorize" in extra and "-ffp-contract=off" in extra
    asm = str(tmp_path / "resize_rgb.s")
    subprocess.check_call([hb.HIPCC, "-x", "hip", *hb.COMMON, *extra, "--cuda-device-only", "-S", os.path.join(hb.CSRC, UNIT), "-o", asm],
                          stderr=subprocess.DEVNULL)
    text = open(asm).read()
    # one YAML entry per kernel, each with a .name and its counts
    entries = re.split(r"\n\s*- \.agpr_count:", text[text.index("amdhsa.kernels"):])[1:]
    seen = {}
    for e in entries:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        meta = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", e)}
        seen[name] = meta
        print(name, meta)
        assert meta["private_segment_fixed_size"] == 0 and meta.get("vgpr_spill_count", 0) == 0 and meta.get("sgpr_spill_count", 0) == 0, name
        assert meta["vgpr_count"] <= 64, name
    assert len(seen) == 3 * len(TAPS)
    for t in TAPS:
        assert sum(f"resize_{t}_kernel" in name for name in seen) == 2, f"both thread maps of the {t} kernel"
        assert sum(f"resize_rois_{t}_kernel" in name for name in seen) == 1, f"the many-regions {t} kernel"
