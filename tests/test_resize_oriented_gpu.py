"""GPU: hp_resize_oriented_u8c3 / hp_resize_oriented_yuv (resize_oriented.hip) for all eight HP_ORIENT_* codes.  The contract: the bytes equal
"convert the whole stored frame to 8-bit BGR by the feed's own rule, orient it (tests/orient_ref.py), then the CPU oracle of hp_resize_u8c3 /
hp_letterbox_u8c3 from the upright size" - and, for BGR, the existing hp_resize_u8c3 on the uploaded upright frame.  Byte equality only; bytes of
the destination outside dw * 3 x dh keep their pre-fill; refused calls launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hdr_ref  # noqa: E402
import orient_ref  # noqa: E402
import yuv_formats_ref as ref  # noqa: E402

from hyperpose_amd import frontend  # noqa: E402
from hyperpose_amd._lib import DevBuf  # noqa: E402
from oracle import loader  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = (3, 250, 77)
PREFILL = 0xA5


def _run(src, dw, dh, code, keep_ratio, **kw):
    """The oriented call into a pre-filled destination with padded rows and a tail: ([dh, dw, 3] picture, every other byte)."""
    dst_stride = dw * 3 + 7
    dst = DevBuf.from_numpy(np.full(dh * dst_stride + 11, PREFILL, np.uint8))
    frontend.resize_oriented(src, dst, dw, dh, code, keep_ratio, FILL, dst_stride=dst_stride, **kw)
    frontend.check(frontend.lib().hp_device_synchronize())
    flat = dst.to_numpy(np.uint8, (dh * dst_stride + 11,))
    rows = flat[:dh * dst_stride].reshape(dh, dst_stride)
    return rows[:, :dw * 3].reshape(dh, dw, 3).copy(), np.concatenate([rows[:, dw * 3:].ravel(), flat[dh * dst_stride:]])


def _assert_same(got, want, what):
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, f"{what}: {len(bad)} pixels differ, first at {bad[0].tolist()}"


def _oracle(upright, dw, dh, keep_ratio):
    return loader.letterbox_u8(upright, dw, dh, bgcolor=FILL) if keep_ratio else loader.resize_linear_u8(upright, dw, dh)


# ---- BGR ------------------------------------------------------------------------------------------------------------------------------

def _bgr(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pitch = w * 3 + 5
    padded = np.full((h, pitch), 0x5A, np.uint8)
    padded[:, :w * 3] = img.reshape(h, w * 3)
    return img, DevBuf.from_numpy(padded), pitch


@pytest.fixture(scope="module")
def frames(hp):
    return {(97, 61): _bgr(97, 61, 21), (96, 60): _bgr(96, 60, 22)}


@pytest.mark.parametrize("code", orient_ref.CODES)
def test_bgr_equals_resize_of_the_upright_frame(hp, frames, code):
    # 97 x 61: odd, non-square, so the last-column one-tap case is met on both axes behind a turn
    uw, uh = orient_ref.oriented_size(code, 97, 61)
    aw, ah = orient_ref.oriented_size(code, 96, 60)
    cases = [((97, 61), 40, 33, False, "linear"), ((97, 61), uw, uh, False, "copy"), ((96, 60), aw // 2, ah // 2, False, "area 2 x 2"),
             ((97, 61), 48, 48, True, "letterbox"), ((97, 61), 150, 131, False, "enlarging"), ((96, 60), 24, 24, True, "letterbox, area or linear")]
    for size, dw, dh, keep_ratio, what in cases:
        img, dev, pitch = frames[size]
        upright = orient_ref.orient(img, code)
        got, rest = _run(dev, dw, dh, code, keep_ratio, sw=size[0], sh=size[1], src_stride=pitch)
        what = f"code {code} {size} -> {dw} x {dh} ({what})"
        assert (rest == PREFILL).all(), what + ": bytes outside dw * 3 x dh were written"
        _assert_same(got, _oracle(upright, dw, dh, keep_ratio), what + " vs the CPU oracle on the upright frame")
        _assert_same(got, frontend.resize_host(upright, dw, dh, keep_ratio, FILL), what + " vs hp_resize_u8c3 on the uploaded upright frame")
        assert upright.tobytes() == frontend.orient_host(img, code).tobytes()


THREAD_MAP_CHILD = """
import os, sys
import numpy as np
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
sys.path.insert(0, sys.argv[1])
import orient_ref
from hyperpose_amd import _lib, frontend
from oracle import loader
_lib.init(0)
img = np.random.default_rng(23).integers(0, 256, (61, 97, 3), dtype=np.uint8)
dev = _lib.DevBuf.from_numpy(img)
for code in orient_ref.CODES:
    up = orient_ref.orient(img, code)
    for dw, dh in [(40, 33), (150, 131), up.shape[1::-1]]:
        dst = _lib.DevBuf.from_numpy(np.full(dw * dh * 3 + 5, 0xA5, np.uint8))
        frontend.resize_oriented(dev, dst, dw, dh, code, sw=97, sh=61)
        _lib.check(_lib.lib().hp_device_synchronize())
        got = dst.to_numpy(np.uint8, (dw * dh * 3 + 5,))
        assert got[:-5].tobytes() == loader.resize_linear_u8(up, dw, dh).tobytes() and (got[-5:] == 0xA5).all(), (os.environ["HP_ORIENT_MAP"], code, dw, dh)
print("MAP_OK", os.environ["HP_ORIENT_MAP"])
"""


@pytest.mark.parametrize("thread_map", ["rows", "cols"])
def test_both_thread_maps_write_the_same_bytes(hp, thread_map):
    """The library picks the per-frame kernels' thread map from the code; HP_ORIENT_MAP (read once per process, hence the child) forces one, so
    that every code runs through both maps: the bytes are the oracle's either way."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", THREAD_MAP_CHILD, root], env=dict(os.environ, HP_ORIENT_MAP=thread_map), capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and out.stdout.split()[-2:] == ["MAP_OK", thread_map], out.stdout[-1500:] + out.stderr[-1500:]


# ---- YUV ------------------------------------------------------------------------------------------------------------------------------

YW, YH = 64, 48
PITCHES = {2: (34, 6), 3: (2, 70, 6), 1: (26,)}  # per plane count; the U and the V plane of a planar frame differ in pitch
DESTS = [(24, 20), (20, 24)]


def _yuv_image(fmt, matrix, range_, seed):
    frame = ref.random_frame(fmt, YW, YH, seed)
    planes = frontend.yuv_planes(frame, fmt, YW, YH)
    bufs, strides = frontend.yuv_upload(planes, fmt, PITCHES[len(planes)], fill=0x5A)
    return frame, frontend.yuv_image(fmt, [b.ptr for b in bufs], strides, YW, YH, matrix, range_), bufs


def _check_yuv(im, bgr, what, tonemap=None):
    for code in orient_ref.CODES:
        upright = orient_ref.orient(bgr, code)
        for (dw, dh) in DESTS:
            for keep_ratio in (False, True):
                got, rest = _run(im, dw, dh, code, keep_ratio, tonemap=tonemap)
                w = f"{what} code {code} -> {dw} x {dh} keep_ratio={keep_ratio}"
                assert (rest == PREFILL).all(), w + ": bytes outside dw * 3 x dh were written"
                _assert_same(got, _oracle(upright, dw, dh, keep_ratio), w)


@pytest.mark.parametrize("fmt", ref.FORMATS)
@pytest.mark.parametrize("matrix,range_", [("bt601", "limited"), ("bt709", "full")])
def test_yuv_equals_convert_orient_resize(hp, fmt, matrix, range_):
    frame, im, keep = _yuv_image(fmt, matrix, range_, 31 + ref.FORMATS.index(fmt))
    _check_yuv(im, ref.to_bgr(frame, fmt, YW, YH, matrix, range_), f"{fmt} {matrix} {range_}")


@pytest.mark.parametrize("fmt,transfer", [("p010", "pq"), ("i010", "hlg")])
def test_hdr_equals_tonemap_orient_resize(hp, fmt, transfer):
    frame, im, keep = _yuv_image(fmt, "bt2020", "limited", 77)
    A, M, O = frontend.tonemap_tables(transfer, True)
    bgr = hdr_ref.to_bgr(frame, fmt, YW, YH, "bt2020", "limited", A, M, O, True)
    tm = frontend.Tonemap(transfer, True)
    try:
        _check_yuv(im, bgr, f"{fmt} {transfer}", tonemap=tm)
    finally:
        frontend.check(frontend.lib().hp_device_synchronize())
        tm.close()


# ---- the identity ---------------------------------------------------------------------------------------------------------------------

def test_orientation_0_equals_the_existing_calls(hp, frames):
    img, dev, pitch = frames[(97, 61)]
    for dw, dh, keep_ratio in [(40, 33, False), (97, 61, False), (48, 48, True)]:
        got, rest = _run(dev, dw, dh, 0, keep_ratio, sw=97, sh=61, src_stride=pitch)
        assert (rest == PREFILL).all()
        _assert_same(got, frontend.resize_host(img, dw, dh, keep_ratio, FILL), f"BGR {dw} x {dh}")
    for fmt in ("nv12", "yuy2", "p010"):
        frame, im, keep = _yuv_image(fmt, "bt709", "limited", 5)
        planes = frontend.yuv_planes(frame, fmt, YW, YH)
        for keep_ratio in (False, True):
            got, rest = _run(im, 24, 20, 0, keep_ratio)
            assert (rest == PREFILL).all()
            _assert_same(got, frontend.resize_yuv_host(planes, 24, 20, fmt, "bt709", "limited", keep_ratio, FILL), f"{fmt} keep_ratio={keep_ratio}")
    frame, im, keep = _yuv_image("p010", "bt2020", "limited", 6)
    tm = frontend.Tonemap("pq", True)
    try:
        for keep_ratio in (False, True):
            got, _ = _run(im, 24, 20, 0, keep_ratio, tonemap=tm)
            want = frontend.resize_yuv_host(frontend.yuv_planes(frame, "p010", YW, YH), 24, 20, "p010", "bt2020", "limited", keep_ratio, FILL, tonemap=tm)
            _assert_same(got, want, f"p010 pq keep_ratio={keep_ratio}")
    finally:
        frontend.check(frontend.lib().hp_device_synchronize())
        tm.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refused_calls_launch_nothing(hp):
    L = hp.lib()
    dw, dh = 16, 12
    sentinel = np.full(dw * 3 * dh, 0xCD, np.uint8)
    dst = DevBuf.from_numpy(sentinel)
    bgr_dev = DevBuf.from_numpy(np.zeros((YH, YW, 3), np.uint8))
    _, nv12, keep1 = _yuv_image("nv12", "bt601", "limited", 1)
    _, p010, keep2 = _yuv_image("p010", "bt2020", "limited", 2)
    tm = frontend.Tonemap("pq", True)

    def bgr(code, src=bgr_dev.ptr, sw=YW, sh=YH, stride=YW * 3, d=dst.ptr, w=dw, h=dh, ds=dw * 3):
        rc = L.hp_resize_oriented_u8c3(src, sw, sh, stride, code, 0, 0, 0, 0, d, w, h, ds, None)
        return rc, L.hp_last_error().decode()

    def yuv(code, im=nv12, t=None, d=dst.ptr, w=dw, h=dh, ds=dw * 3):
        rc = L.hp_resize_oriented_yuv(C.byref(im), t, code, 1, 0, 0, 0, d, w, h, ds, None)
        return rc, L.hp_last_error().decode()

    try:
        for code in (8, -1, 100):
            for rc, msg in (bgr(code), yuv(code), yuv(code, p010, tm.h)):
                assert rc == hp.HP_ERR_INVALID and "orientation" in msg, (rc, msg)
        bad_frame = frontend.yuv_image("nv12", [nv12.plane[0], nv12.plane[1]], [YW - 2, nv12.stride[1]], YW, YH)
        odd_frame = frontend.yuv_image("nv12", [nv12.plane[0], nv12.plane[1]], [nv12.stride[0], nv12.stride[1]], YW - 1, YH)
        for code in (0, 1, 6):  # whatever the un-oriented twin refuses, through the identity's forward and through the oriented path
            refused = [bgr(code, src=None), bgr(code, sw=0), bgr(code, stride=YW * 3 - 1), bgr(code, d=None), bgr(code, w=0), bgr(code, ds=dw * 3 - 1),
                       yuv(code, bad_frame), yuv(code, odd_frame), yuv(code, d=None), yuv(code, ds=dw * 3 - 1), yuv(code, p010, tm.h, h=0)]
            for rc, msg in refused:
                assert rc == hp.HP_ERR_INVALID and len(msg) > 0, (code, rc, msg)
            rc, msg = yuv(code, nv12, tm.h)  # an 8-bit layout with a tone-map
            assert rc == hp.HP_ERR_INVALID and "HP_YUV_NV12" in msg, (code, rc, msg)
            assert "HP_YUV_NV12" in yuv(code, bad_frame)[1]
        hp.check(L.hp_device_synchronize())
        assert np.array_equal(dst.to_numpy(np.uint8, sentinel.shape), sentinel), "a refused call wrote to the destination"
        assert bgr(5)[0] == hp.HP_OK and yuv(3)[0] == hp.HP_OK and yuv(7, p010, tm.h)[0] == hp.HP_OK
        hp.check(L.hp_device_synchronize())
    finally:
        tm.close()
