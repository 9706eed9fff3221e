"""GPU: hp_scale_stage_u8c3 and hp_scale_merge against their host twins, bit for bit; nothing outside their outputs is written and their inputs
stay as they were; the refusals launch nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flip_ref import special_maps  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, DevBuf, HpError  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
# 3 slots of 88 x 56 over 22 x 14 maps: 0.5 -> 44 x 28 (the 2 x 2 area mode), 0.72 -> 64 x 40 (linear), 1.0 -> 88 x 56 (copy); 0.55 -> 48 x 32
# (linear); over 11 x 7 maps: 0.5 -> 48 x 32
STAGES = [(22, 14, (0.5, 0.72, 1.0)), (22, 14, (0.55,)), (11, 7, (0.5, 0.1))]
# (n, C, H, W, scales): the host cases, and a plane above 256 elements with C = 38
MERGES = [(2, 3, 5, 7, (0.55, 0.1)), (1, 2, 17, 19, (0.75,)), (2, 1, 6, 9, (1.0, 0.5, 0.3)), (2, 38, 17, 19, (0.5,))]


@pytest.mark.parametrize("map_w,map_h,scales", STAGES)
def test_stage_equals_host_twin_and_stays_inside_dst(hp, map_w, map_h, scales):
    n, w, h, fill = 3, 88, 56, (7, 200, 31)
    slots = np.random.default_rng(map_w + len(scales)).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    src_bytes, dst_bytes = slots.size, len(scales) * slots.size
    # [guard | src | dst | guard] in one allocation
    host = np.concatenate([np.full(GUARD, 0xA5, np.uint8), slots.ravel(), np.full(dst_bytes, 0x3C, np.uint8), np.full(GUARD, 0x5A, np.uint8)])
    buf = DevBuf.from_numpy(host)
    base = buf.ptr.value
    frontend.scale_stage(base + GUARD, base + GUARD + src_bytes, w, h, n, map_w, map_h, scales, fill)
    hp.check(hp.lib().hp_device_synchronize())
    got = buf.to_numpy(np.uint8, host.shape)
    want = frontend.scale_stage_host(slots, map_w, map_h, scales, fill)
    assert got[GUARD + src_bytes:GUARD + src_bytes + dst_bytes].tobytes() == want.tobytes()
    assert got[:GUARD + src_bytes].tobytes() == host[:GUARD + src_bytes].tobytes()  # the guard and the source are untouched
    assert got[GUARD + src_bytes + dst_bytes:].tobytes() == host[GUARD + src_bytes + dst_bytes:].tobytes()


@pytest.mark.parametrize("n,C_,H,W,scales", MERGES)
def test_merge_equals_host_twin_and_writes_only_the_first_n_maps(hp, n, C_, H, W, scales):
    K = len(scales) + 1
    maps = special_maps(np.random.default_rng(100 * H + W + C_), (K * n, C_, H, W))
    host = np.concatenate([maps.ravel(), np.full(GUARD, 7.25, np.float32)])
    dev = DevBuf.from_numpy(host)
    frontend.scale_merge(dev, n, K, C_, H, W, scales)
    hp.check(hp.lib().hp_device_synchronize())
    got = dev.to_numpy(np.float32, host.shape)
    want = frontend.scale_merge_host(maps, n, scales)
    assert got[:maps.size].tobytes() == want.ravel().tobytes()
    assert got[n * C_ * H * W:].tobytes() == host[n * C_ * H * W:].tobytes()  # the maps behind n and the guard band
    assert got[:n * C_ * H * W].tobytes() != maps[:n].tobytes()


def test_merge_refusals_launch_nothing(hp):
    maps = special_maps(np.random.default_rng(3), (2, 4, 2, 3))
    dev = DevBuf.from_numpy(maps)
    for what, args in [("K 1", (1, 1, 4, 2, 3, [])), ("K 5", (1, 5, 4, 2, 3, [0.5] * 4)), ("scale 0 ", (1, 2, 4, 2, 3, [0.0])),
                       ("scale 2", (1, 2, 4, 2, 3, [2.0])), ("scale nan", (1, 2, 4, 2, 3, [float("nan")])), ("C 0", (1, 2, 0, 2, 3, [0.5])),
                       ("C 257", (1, 2, 257, 2, 3, [0.5])), ("H 0", (1, 2, 4, 0, 3, [0.5])), ("W -2", (1, 2, 4, 2, -2, [0.5])),
                       ("H 65536 x W 65536", (1, 2, 4, 65536, 65536, [0.5])), ("n 0", (0, 2, 4, 2, 3, [0.5])), ("n 65536", (65536, 2, 4, 2, 3, [0.5]))]:
        with pytest.raises(HpError) as e:
            frontend.scale_merge(dev, *args)
        assert e.value.code == HP_ERR_INVALID and what in str(e.value), str(e.value)
    hp.check(hp.lib().hp_device_synchronize())
    assert dev.to_numpy(np.float32, maps.shape).tobytes() == maps.tobytes()


def test_stage_refusals_launch_nothing(hp):
    slots = np.zeros((1, 56, 88, 3), np.uint8)
    buf = DevBuf.from_numpy(np.concatenate([slots.ravel(), np.full(slots.size, 0x3C, np.uint8)]))
    base = buf.ptr.value
    for what, kw in [("not a whole number of map cells", dict(map_w=10)), ("n_scales 0", dict(scales=[])), ("scale 1.5", dict(scales=[1.5])),
                     ("fill (300, 0, 0)", dict(bgcolor=(300, 0, 0))), ("overlap", dict(dst=base + 88 * 3))]:
        args = dict(src=base, dst=base + slots.size, map_w=11, scales=[0.5], bgcolor=(0, 0, 0))
        args.update(kw)
        with pytest.raises(HpError) as e:
            frontend.scale_stage(args["src"], args["dst"], 88, 56, 1, args["map_w"], 7, args["scales"], args["bgcolor"])
        assert e.value.code == HP_ERR_INVALID and what in str(e.value), str(e.value)
    hp.check(hp.lib().hp_device_synchronize())
    assert np.all(buf.to_numpy(np.uint8, (2 * slots.size,))[slots.size:] == 0x3C)
