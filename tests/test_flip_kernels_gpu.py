"""GPU: hp_hflip_u8c3 and hp_flip_merge against their host twins, bit for bit; nothing outside their outputs is written; merging synthetic PAF maps
with their exact mirror image returns the maps, and the parser reads the same humans from both."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flip_ref import special_maps, tables  # noqa: E402

from hyperpose_amd import frontend, synth  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, DevBuf, HpError  # noqa: E402
from hyperpose_amd.parser import Paf  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 1, 2), (19, 2, 5), (38, 3, 7), (5, 4, 65), (256, 1, 3)]
CANARY = 64


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h", [1, 3])
@pytest.mark.parametrize("w", [1, 2, 3, 17, 69])
def test_hflip_equals_host_twin_and_stays_inside_dst(hp, w, h, n):
    rng = np.random.default_rng(w * 100 + h * 10 + n)
    frames = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    size = frames.size
    # [canary | src | dst | canary] in one allocation: dst == src + n * w * h * 3, the expected use, at whatever alignment that gives
    host = np.concatenate([np.full(CANARY, 0xA5, np.uint8), frames.ravel(), np.full(size, 0x3C, np.uint8), np.full(CANARY, 0x5A, np.uint8)])
    buf = DevBuf.from_numpy(host)
    frontend.hflip_u8c3(buf.ptr.value + CANARY, buf.ptr.value + CANARY + size, w, h, n)
    hp.check(hp.lib().hp_device_synchronize())
    got = buf.to_numpy(np.uint8, host.shape)
    assert got[CANARY + size:CANARY + 2 * size].tobytes() == frontend.hflip_u8c3_host(frames).tobytes()
    assert got[:CANARY + size].tobytes() == host[:CANARY + size].tobytes() and got[CANARY + 2 * size:].tobytes() == host[CANARY + 2 * size:].tobytes()


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_merge_equals_host_twin_and_writes_only_the_first_n_maps(hp, shape, n):
    rng = np.random.default_rng(1000 * n + sum(shape))
    maps = special_maps(rng, (2 * n + 1,) + shape)
    perm, sign = tables(rng, shape[0])
    dev = DevBuf.from_numpy(maps)
    frontend.flip_merge(dev, n, *shape, perm, sign)
    hp.check(hp.lib().hp_device_synchronize())
    got = dev.to_numpy(np.float32, maps.shape)
    assert got.tobytes() == frontend.flip_merge_host(maps, n, perm, sign).tobytes()
    assert got[n:].tobytes() == maps[n:].tobytes()
    assert got[:n].tobytes() != maps[:n].tobytes() or shape == (1, 1, 1)


def test_merge_refusals_launch_nothing(hp):
    maps = special_maps(np.random.default_rng(3), (3, 4, 2, 3))
    dev = DevBuf.from_numpy(maps)
    perm, sign = np.arange(4, dtype=np.int32), np.ones(4, np.int8)
    for what, args in [("C 0", (1, 0, 2, 3, perm, sign)), ("C 257", (1, 257, 2, 3, np.arange(257, dtype=np.int32), np.ones(257, np.int8))),
                       ("perm[1] = 7", (1, 4, 2, 3, np.array([0, 7, 2, 3], np.int32), sign)), ("sign[0] = 0", (1, 4, 2, 3, perm, np.array([0, 1, 1, 1], np.int8))),
                       ("n 0", (0, 4, 2, 3, perm, sign)), ("H 0", (1, 4, 0, 3, perm, sign)), ("W -2", (1, 4, 2, -2, perm, sign))]:
        with pytest.raises(HpError) as e:
            frontend.flip_merge(dev, *args)
        assert e.value.code == HP_ERR_INVALID and what in str(e.value), str(e.value)
    hp.check(hp.lib().hp_device_synchronize())
    assert dev.to_numpy(np.float32, maps.shape).tobytes() == maps.tobytes()


def test_maps_merged_with_their_mirror_image_parse_to_the_same_humans(hp):
    n = 2
    conf, paf, _ = synth.paf_maps(synth.rng_for(1, salt=91), n, rows=23, cols=27, people=(2, 3), scale_range=(8.0, 14.0))
    conf_perm, paf_perm, paf_sign = frontend.flip_tables_coco(19)
    conf_sign = np.ones(19, np.int8)
    # [maps, their exact mirror image, one map more]: a + a and 0.5 * 2a are exact, so the merge must return the maps themselves
    both = []
    for m, perm, sign in ((conf, conf_perm, conf_sign), (paf, paf_perm, paf_sign)):
        mirror = np.ascontiguousarray((m[:, perm] * sign[None, :, None, None].astype(np.float32))[..., ::-1])
        both.append(np.concatenate([m, mirror, m[:1]]))
    dconf, dpaf = DevBuf.from_numpy(both[0]), DevBuf.from_numpy(both[1])
    frontend.flip_merge(dconf, n, *conf.shape[1:], conf_perm, conf_sign)
    frontend.flip_merge(dpaf, n, *paf.shape[1:], paf_perm, paf_sign)
    hp.check(hp.lib().hp_device_synchronize())
    assert dconf.to_numpy(np.float32, both[0].shape).tobytes() == both[0].tobytes()
    assert dpaf.to_numpy(np.float32, both[1].shape).tobytes() == both[1].tobytes()
    parser = Paf(max_batch=n)
    merged = parser.process_batch_device(dconf, dpaf, n, conf.shape[1:], paf.shape[1:])
    original = parser.process_batch_device(DevBuf.from_numpy(conf), DevBuf.from_numpy(paf), n, conf.shape[1:], paf.shape[1:])
    assert sum(len(f) for f in original) >= 1
    for a, b in zip(merged, original):
        assert a.tobytes() == b.tobytes()
