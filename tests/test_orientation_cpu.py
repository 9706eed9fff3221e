"""CPU: the host side of HP_ORIENT_* (hp_oriented_size, hp_orientation_from_exif, hp_orient_roi, hp_orient_u8c3_host, hp_humans_orient) against
its numpy restatement (tests/orient_ref.py).  Every comparison is byte or bit equality; no device is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

import orient_ref
from hyperpose_amd import _lib, frontend
from hyperpose_amd._lib import HP_ERR_INVALID, HUMAN_DTYPE, HpError, Human, Roi


def _stored(w, h, seed, pitch):
    """A stored [h, w, 3] frame as a view of rows padded by `pitch` bytes."""
    rows = np.random.default_rng(seed).integers(0, 256, (h, w * 3 + pitch), dtype=np.uint8)
    return rows[:, :w * 3].reshape(h, w, 3)


@pytest.mark.parametrize("w,h", [(7, 5), (1, 4)])
@pytest.mark.parametrize("code", orient_ref.CODES)
def test_orient_host_equals_the_restatement(w, h, code):
    S = _stored(w, h, 10 * w + code, pitch=5)
    want = orient_ref.orient(S, code)
    assert np.array_equal(want, orient_ref.orient_by_map(S, code)), "the two restatements disagree"
    got = frontend.orient_host(S, code, dst_pitch=7)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()
    assert (got.base[:, got.shape[1] * 3:] == 0xA5).all(), "padding bytes of the destination were written"


def test_the_eight_results_of_an_asymmetric_frame_differ():
    S = _stored(7, 5, 99, pitch=0)
    out = [frontend.orient_host(S, c) for c in orient_ref.CODES]
    for a, b in itertools.combinations(range(8), 2):
        assert out[a].shape != out[b].shape or out[a].tobytes() != out[b].tobytes(), (a, b)
    assert out[0].tobytes() == np.ascontiguousarray(S).tobytes()


@pytest.mark.parametrize("code", orient_ref.CODES)
def test_sizes_and_regions(code):
    for sw, sh in [(7, 5), (1, 4), (64, 48)]:
        uw, uh = frontend.oriented_size(code, sw, sh)
        assert (uw, uh) == orient_ref.oriented_size(code, sw, sh)
        # the whole frame, one pixel in each corner, regions touching each edge, an inner one
        rois = [(0, 0, uw, uh), (0, 0, 1, 1), (uw - 1, 0, 1, 1), (0, uh - 1, 1, 1), (uw - 1, uh - 1, 1, 1), (0, 0, 1, uh), (uw - 1, 0, 1, uh),
                (0, 0, uw, 1), (0, uh - 1, uw, 1)]
        if uw > 3 and uh > 3:
            rois += [(1, 2, uw - 3, uh - 3), (uw - 2, uh - 3, 2, 2), (0, 1, 2, uh - 1)]
        S = np.arange(sw * sh, dtype=np.int64).reshape(sh, sw)
        U = orient_ref.orient(S, code)
        for r in rois:
            x, y, w, h = got = frontend.orient_roi(r, code, sw, sh)
            assert got == orient_ref.orient_roi(r, code, sw, sh), (r, got)
            # the stored rectangle holds exactly the upright region's pixels
            assert np.array_equal(orient_ref.orient(S[y:y + h, x:x + w], code), U[r[1]:r[1] + r[3], r[0]:r[0] + r[2]])


def test_exif_table():
    assert [frontend.orientation_from_exif(e) for e in range(1, 9)] == [0, 4, 2, 6, 7, 1, 5, 3] == [orient_ref.EXIF[e] for e in range(1, 9)]
    for bad in (0, 9, -1):
        with pytest.raises(HpError) as e:
            frontend.orientation_from_exif(bad)
        assert e.value.code == HP_ERR_INVALID and "exif" in str(e.value)


def _humans(seed, n=5):
    rng = np.random.default_rng(seed)
    hs = np.zeros(n, HUMAN_DTYPE)
    hs["parts"]["has_value"] = rng.integers(0, 2, (n, 18))
    hs["parts"]["x"] = rng.random((n, 18), dtype=np.float32)
    hs["parts"]["y"] = rng.random((n, 18), dtype=np.float32)
    hs["parts"]["score"] = rng.random((n, 18), dtype=np.float32)
    hs["score"] = rng.random(n, dtype=np.float32)
    hs["parts"]["x"][0, :4] = [0.0, 1.0, 0.5, np.float32(1e-9)]  # the ends, and a value 1.0f - t swallows
    hs["parts"]["has_value"][0, :4] = 1
    return hs


@pytest.mark.parametrize("code", orient_ref.CODES)
@pytest.mark.parametrize("to_stored", [True, False])
def test_humans_orient_equals_the_fp32_formulas(code, to_stored):
    hs = _humans(40 + code)
    got = frontend.humans_orient(hs, code, to_stored)
    want = orient_ref.humans_orient(hs, code, to_stored)
    assert got.tobytes() == want.tobytes()
    absent = hs["parts"]["has_value"] == 0
    assert absent.any() and got["parts"][absent].tobytes() == hs["parts"][absent].tobytes(), "a part without has_value was touched"
    assert got["parts"]["score"].tobytes() == hs["parts"]["score"].tobytes() and got["score"].tobytes() == hs["score"].tobytes()
    if code == 0:
        assert got.tobytes() == hs.tobytes()


@pytest.mark.parametrize("code", orient_ref.CODES)
def test_humans_follow_the_pixels(code):
    """A part at the centre of stored pixel (x, y) of a 8 x 4 frame lands, upright, at the centre of the pixel the frame's map sends there
    (coordinates k / 16 and k / 8 are exact in fp32, and so is 1.0f minus them)."""
    sw, sh = 8, 4
    uw, uh = orient_ref.oriented_size(code, sw, sh)
    for ux, uy in itertools.product(range(uw), range(uh)):
        x, y = orient_ref.stored_xy(code, sw, sh, ux, uy)
        hs = np.zeros(1, HUMAN_DTYPE)
        hs["parts"]["has_value"][0, 0] = 1
        hs["parts"]["x"][0, 0], hs["parts"]["y"][0, 0] = (ux + 0.5) / uw, (uy + 0.5) / uh
        st = frontend.humans_orient(hs, code, True)
        assert (st["parts"]["x"][0, 0], st["parts"]["y"][0, 0]) == (np.float32((x + 0.5) / sw), np.float32((y + 0.5) / sh))
        assert frontend.humans_orient(st, code, False).tobytes() == hs.tobytes()


def test_refusals():
    L = _lib.lib()
    uw, uh = C.c_int(-7), C.c_int(-7)
    src, dst = np.zeros((5, 7 * 3), np.uint8), np.full((7, 7 * 3), 0xA5, np.uint8)
    u, st = Roi(0, 0, 2, 2), Roi(-7, -7, -7, -7)
    hs = _humans(1)
    before = hs.copy()
    hp_ = hs.ctypes.data_as(C.POINTER(Human))
    sp, dp = C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data)
    calls = [
        ("orientation", lambda: L.hp_oriented_size(8, 7, 5, C.byref(uw), C.byref(uh))),
        ("orientation", lambda: L.hp_oriented_size(-1, 7, 5, C.byref(uw), C.byref(uh))),
        ("empty", lambda: L.hp_oriented_size(1, 0, 5, C.byref(uw), C.byref(uh))),
        ("empty", lambda: L.hp_oriented_size(1, 7, -5, C.byref(uw), C.byref(uh))),
        ("null", lambda: L.hp_oriented_size(1, 7, 5, None, C.byref(uh))),
        ("orientation", lambda: L.hp_orient_roi(C.byref(u), 8, 7, 5, C.byref(st))),
        ("null", lambda: L.hp_orient_roi(None, 1, 7, 5, C.byref(st))),
        ("null", lambda: L.hp_orient_roi(C.byref(u), 1, 7, 5, None)),
        ("region", lambda: L.hp_orient_roi(C.byref(Roi(0, 0, 7, 5)), 1, 7, 5, C.byref(st))),  # the upright frame is 5 x 7
        ("region", lambda: L.hp_orient_roi(C.byref(Roi(4, 0, 2, 2)), 1, 7, 5, C.byref(st))),
        ("region", lambda: L.hp_orient_roi(C.byref(Roi(0, 0, 0, 2)), 0, 7, 5, C.byref(st))),
        ("region", lambda: L.hp_orient_roi(C.byref(Roi(-1, 0, 2, 2)), 0, 7, 5, C.byref(st))),
        ("orientation", lambda: L.hp_orient_u8c3_host(sp, 7, 5, 21, 9, dp, 21)),
        ("null", lambda: L.hp_orient_u8c3_host(None, 7, 5, 21, 1, dp, 21)),
        ("null", lambda: L.hp_orient_u8c3_host(sp, 7, 5, 21, 1, None, 21)),
        ("src_stride", lambda: L.hp_orient_u8c3_host(sp, 7, 5, 20, 1, dp, 21)),
        ("dst_stride", lambda: L.hp_orient_u8c3_host(sp, 7, 5, 21, 1, dp, 14)),  # an upright row is 5 pixels
        ("dst_stride", lambda: L.hp_orient_u8c3_host(sp, 7, 5, 21, 2, dp, 20)),
        ("empty", lambda: L.hp_orient_u8c3_host(sp, 0, 5, 21, 1, dp, 21)),
        ("orientation", lambda: L.hp_humans_orient(hp_, len(hs), 8, 1)),
        ("orientation", lambda: L.hp_humans_orient(hp_, len(hs), -1, 0)),
        ("null", lambda: L.hp_humans_orient(None, 2, 1, 1)),
        ("humans", lambda: L.hp_humans_orient(hp_, -1, 1, 1)),
    ]
    for word, call in calls:
        rc = call()
        msg = L.hp_last_error().decode()
        assert rc == HP_ERR_INVALID and word in msg, (word, rc, msg)
    assert (uw.value, uh.value) == (-7, -7) and (st.x, st.y, st.w, st.h) == (-7, -7, -7, -7)
    assert (dst == 0xA5).all() and hs.tobytes() == before.tobytes(), "a refused call wrote"
    # what the refusals were derived from is accepted
    assert L.hp_orient_u8c3_host(sp, 7, 5, 21, 1, dp, 15) == 0 and L.hp_humans_orient(None, 0, 7, 1) == 0
    assert L.hp_orient_roi(C.byref(Roi(3, 5, 2, 2)), 1, 7, 5, C.byref(st)) == 0 and (st.x, st.y, st.w, st.h) == orient_ref.orient_roi((3, 5, 2, 2), 1, 7, 5)
