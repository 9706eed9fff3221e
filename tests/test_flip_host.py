"""hp_flip_merge_host and hp_hflip_u8c3_host (plain C++, no device) against NumPy, bit for bit, and every refusal of the two calls."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from flip_ref import numpy_merge, special_maps, tables  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, HpError  # noqa: E402

SHAPES = [(1, 1, 1), (3, 1, 2), (19, 2, 5), (38, 3, 7), (5, 4, 65), (256, 1, 3)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_merge_host_equals_numpy(shape, n):
    rng = np.random.default_rng(1000 * n + sum(shape))
    maps = special_maps(rng, (2 * n + 1,) + shape)
    perm, sign = tables(rng, shape[0])
    got = frontend.flip_merge_host(maps, n, perm, sign)
    assert got.tobytes() == numpy_merge(maps, n, perm, sign).tobytes()
    assert got[n:].tobytes() == maps[n:].tobytes()  # the flipped maps and what lies behind them are not written


def test_a_map_merged_with_its_exact_mirror_is_unchanged():
    rng = np.random.default_rng(7)
    conf_perm, perm, sign = frontend.flip_tables_coco(19)
    a = special_maps(rng, (2, 38, 5, 9))
    flat = a.reshape(-1)
    flat[np.abs(flat) > 1e20] = np.float32(1.5)  # (2a must stay finite for a + a to be exact)
    mirror = (a[:, perm] * sign[None, :, None, None].astype(np.float32))[..., ::-1]
    got = frontend.flip_merge_host(np.concatenate([a, mirror]), 2, perm, sign)
    # a + a and 0.5 * 2a are exact, denormals included, and zeros keep their sign: -0 + -0 = -0, and -0 - (+0) = -0
    assert got[:2].tobytes() == a.tobytes()


@pytest.mark.parametrize("w,h,n", [(1, 1, 1), (1, 3, 2), (2, 1, 1), (3, 2, 3), (17, 3, 1), (69, 2, 2)])
def test_hflip_host_equals_numpy(w, h, n):
    x = np.random.default_rng(w * 100 + h * 10 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    assert frontend.hflip_u8c3_host(x).tobytes() == np.ascontiguousarray(x[:, :, ::-1]).tobytes()
    assert frontend.hflip_u8c3_host(x[0]).tobytes() == np.ascontiguousarray(x[0][:, ::-1]).tobytes()


def _refused(what, fn):
    with pytest.raises(HpError) as e:
        fn()
    assert e.value.code == HP_ERR_INVALID and what in str(e.value), str(e.value)


def test_merge_host_refusals():
    maps = np.zeros((3, 4, 2, 3), np.float32)
    perm, sign = np.arange(4, dtype=np.int32), np.ones(4, np.int8)
    big = np.arange(257, dtype=np.int32)
    _refused("C 0", lambda: frontend.flip_merge_host(maps, 1, perm, sign, shape=(0, 2, 3)))
    _refused("C 257", lambda: frontend.flip_merge_host(np.zeros((2, 257, 1, 1), np.float32), 1, big, np.ones(257, np.int8)))
    _refused("perm[2] = 4", lambda: frontend.flip_merge_host(maps, 1, np.array([0, 1, 4, 3], np.int32), sign))
    _refused("perm[0] = -1", lambda: frontend.flip_merge_host(maps, 1, np.array([-1, 1, 2, 3], np.int32), sign))
    _refused("sign[1] = 0", lambda: frontend.flip_merge_host(maps, 1, perm, np.array([1, 0, 1, 1], np.int8)))
    _refused("sign[3] = 2", lambda: frontend.flip_merge_host(maps, 1, perm, np.array([1, 1, 1, 2], np.int8)))
    _refused("n 0", lambda: frontend.flip_merge_host(maps, 0, perm, sign))
    _refused("n -1", lambda: frontend.flip_merge_host(maps, -1, perm, sign))
    _refused("H 0", lambda: frontend.flip_merge_host(maps, 1, perm, sign, shape=(4, 0, 3)))
    _refused("W 0", lambda: frontend.flip_merge_host(maps, 1, perm, sign, shape=(4, 2, 0)))
    assert not maps.any()


def test_hflip_host_refusals():
    import ctypes as C
    from hyperpose_amd._lib import lib
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    call = lambda src, dst, w, h, n: lib().hp_hflip_u8c3_host(C.c_void_p(src), C.c_void_p(dst), w, h, n)
    for args in [(p, p + 32, 0, 1, 1), (p, p + 32, 1, 0, 1), (p, p + 32, 1, 1, 0), (None, p, 1, 1, 1), (p, None, 1, 1, 1),
                 (p, p + 3, 2, 1, 1), (p + 3, p, 2, 1, 1), (p, p, 1, 1, 1)]:  # the last three: src and dst overlap
        assert call(*args) == HP_ERR_INVALID, args
    assert call(p, p + 6, 2, 1, 1) == 0  # dst == src + n * w * h * 3 is the expected use
