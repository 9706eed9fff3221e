"""hp_scale_tables, hp_scale_merge_host and hp_scale_stage_u8c3_host (plain C++, no device) against NumPy and the restated cv::resize, bit for bit,
and every refusal of the calls."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scale_ref  # noqa: E402
from flip_ref import special_maps  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import HP_ERR_INVALID, HpError, lib  # noqa: E402
from oracle import loader  # noqa: E402

# (n, C, H, W, scales): 5 x 7 maps with valid regions 3 x 4 (0.55) and 1 x 1 (0.1), K = 3; a 17 x 19 plane, K = 2; K = 4 with the identity scale
MERGE_CASES = [(2, 3, 5, 7, (0.55, 0.1)), (1, 2, 17, 19, (0.75,)), (2, 1, 6, 9, (1.0, 0.5, 0.3))]


@pytest.mark.parametrize("W,mw", [(7, 4), (7, 1), (11, 6), (54, 27), (54, 41), (5, 5)])
def test_tables_equal_the_restatement(W, mw):
    idx, wgt = frontend.scale_tables(W, mw)
    ridx, rwgt = scale_ref.tables(W, mw)
    assert idx.tobytes() == ridx.tobytes() and wgt.tobytes() == rwgt.tobytes()
    assert idx.min() >= 0 and idx.max() <= mw - 1


def test_identity_tables_are_exactly_one_tap():
    idx, wgt = frontend.scale_tables(5, 5)
    assert wgt.tobytes() == np.tile(np.array([0, 1, 0, 0], np.float32), (5, 1)).tobytes()  # +0 zeros: every term is exact
    assert np.array_equal(idx[:, 1], np.arange(5))


def test_cells_round_to_whole_map_cells():
    assert [scale_ref.cells(s, 7) for s in (0.55, 0.1, 1.0)] == [4, 1, 7]
    assert [scale_ref.cells(s, 5) for s in (0.55, 0.1, 1.0)] == [3, 1, 5]


@pytest.mark.parametrize("n,C_,H,W,scales", MERGE_CASES)
def test_merge_host_equals_numpy(n, C_, H, W, scales):
    K = len(scales) + 1
    maps = special_maps(np.random.default_rng(100 * H + W), (K * n + 1, C_, H, W))
    got = frontend.scale_merge_host(maps, n, scales)
    assert got.tobytes() == scale_ref.merge(maps, n, scales).tobytes()
    assert got[n:].tobytes() == maps[n:].tobytes()  # the shrunken passes' maps and what lies behind them are not written
    assert got[:n].tobytes() != maps[:n].tobytes()


def test_merge_reads_only_the_valid_region():
    n, scales = 2, (0.55, 0.1)
    maps = special_maps(np.random.default_rng(5), (3 * n, 3, 5, 7))
    dirty = maps.copy()
    dirty[n:2 * n, :, 3:, :] = np.nan  # outside 3 x 4 at 0.55
    dirty[n:2 * n, :, :, 4:] = np.nan
    dirty[2 * n:, :, 1:, :] = np.inf  # outside 1 x 1 at 0.1
    dirty[2 * n:, :, :, 1:] = np.inf
    assert frontend.scale_merge_host(dirty, n, scales)[:n].tobytes() == frontend.scale_merge_host(maps, n, scales)[:n].tobytes()


def _refused(what, fn):
    with pytest.raises(HpError) as e:
        fn()
    assert e.value.code == HP_ERR_INVALID and what in str(e.value), str(e.value)


def test_tables_refusals():
    _refused("W 0", lambda: frontend.scale_tables(0, 1))
    _refused("mw 0", lambda: frontend.scale_tables(5, 0))
    _refused("mw 6 (1 .. W = 5)", lambda: frontend.scale_tables(5, 6))
    assert lib().hp_scale_tables(5, 5, None, None) == HP_ERR_INVALID and "null" in lib().hp_last_error().decode()


def test_merge_host_refusals():
    maps = np.zeros((4, 2, 3, 5), np.float32)
    m = lambda *a, **k: (lambda: frontend.scale_merge_host(maps, *a, **k))
    _refused("K 1", m(1, [], K=1))
    _refused("K 5", m(1, [0.5, 0.5, 0.5, 0.5]))
    _refused("scale 0 ", m(1, [0.0]))
    _refused("scale 1.5", m(1, [1.5]))
    _refused("scale -0.5", m(1, [-0.5]))
    _refused("scale nan", m(1, [float("nan")]))
    _refused("scale inf", m(1, [float("inf")]))
    _refused("scales[1]", m(1, [0.5, 2.0]))
    _refused("C 0", m(1, [0.5], shape=(0, 3, 5)))
    _refused("C 257", m(1, [0.5], shape=(257, 3, 5)))
    _refused("H 0", m(1, [0.5], shape=(2, 0, 5)))
    _refused("W 0", m(1, [0.5], shape=(2, 3, 0)))
    _refused("H 65536 x W 65536", m(1, [0.5], shape=(2, 65536, 65536)))
    _refused("n 0", m(0, [0.5]))
    _refused("n -1", m(-1, [0.5]))
    _refused("n 65536", m(65536, [0.5]))
    assert lib().hp_scale_merge_host(None, 1, 2, 1, 1, 1, (C.c_float * 1)(0.5)) == HP_ERR_INVALID
    assert not maps.any()


def _slot_reference(slot, iw, ih, fill):
    h, w, _ = slot.shape
    out = np.empty_like(slot)
    out[:] = np.array(fill, np.uint8)
    out[:ih, :iw] = loader.resize_linear_u8(slot, iw, ih)
    return out


# 88 x 56 slots over 22 x 14 maps (cells of 4 x 4 pixels): 0.5 -> 44 x 28 (the 2 x 2 area mode), 0.55 -> 48 x 32 and 0.72 -> 64 x 40 (linear),
# 1.0 -> 88 x 56 (copy); over 11 x 7 maps (cells of 8 x 8): 0.5 -> 48 x 32, 0.1 -> 8 x 8
@pytest.mark.parametrize("map_w,map_h,scales,inner", [(22, 14, (0.5, 0.72, 1.0), [(44, 28), (64, 40), (88, 56)]),
                                                      (22, 14, (0.55,), [(48, 32)]), (11, 7, (0.5, 0.1), [(48, 32), (8, 8)])])
def test_stage_host_equals_resize_then_paste(map_w, map_h, scales, inner):
    n, fill = 3, (7, 200, 31)
    slots = np.random.default_rng(map_w + len(scales)).integers(0, 256, (n, 56, 88, 3), dtype=np.uint8)
    got = frontend.scale_stage_host(slots, map_w, map_h, scales, fill)
    assert got.shape == (len(scales) * n, 56, 88, 3)
    for k, (iw, ih) in enumerate(inner):
        assert (scale_ref.cells(scales[k], map_w) * 88 // map_w, scale_ref.cells(scales[k], map_h) * 56 // map_h) == (iw, ih)
        for i in range(n):
            assert got[k * n + i].tobytes() == _slot_reference(slots[i], iw, ih, fill).tobytes(), (k, i)
    assert got[-1].tobytes() != slots[-1].tobytes() or scales[-1] == 1.0


def test_stage_host_refusals():
    buf = np.zeros(2 * 88 * 56 * 3 * 4, np.uint8)
    p = buf.ctypes.data
    slot = 88 * 56 * 3
    s = lambda *v: (C.c_float * max(1, len(v)))(*v)

    def call(src, dst, w=88, h=56, n=1, mw=11, mh=7, scales=s(0.5), k=1, b=0, g=0, r=0):
        return lib().hp_scale_stage_u8c3_host(C.c_void_p(src), C.c_void_p(dst), w, h, n, mw, mh, scales, k, b, g, r)

    assert call(p, p + slot) == 0
    for what, kw in [("is not a whole number of map cells of 10 x 7", dict(mw=10)), ("88 x 57", dict(h=57)), ("n_scales 0", dict(k=0)),
                     ("n_scales 4", dict(k=4, scales=s(0.5, 0.5, 0.5, 0.5))), ("scale 0 ", dict(scales=s(0.0))), ("scale 1.25", dict(scales=s(1.25))),
                     ("scales[1]", dict(k=2, scales=s(0.5, float("nan")))), ("fill (256, 0, 0)", dict(b=256)), ("fill (0, 0, -1)", dict(r=-1)),
                     ("n 0", dict(n=0)), ("map_w 0", dict(mw=0)), ("more than 65535 slots", dict(n=30000, k=3, scales=s(0.5, 0.5, 0.5)))]:
        assert call(p, p + 2 * slot, **kw) == HP_ERR_INVALID, what
        assert what in lib().hp_last_error().decode(), (what, lib().hp_last_error())
    assert call(p, p + slot // 2) == HP_ERR_INVALID and "overlap" in lib().hp_last_error().decode()
    assert call(p + slot, p, n=1, k=2, scales=s(0.5, 0.5)) == HP_ERR_INVALID  # dst's two slots run into src
    assert call(None, p) == HP_ERR_INVALID
