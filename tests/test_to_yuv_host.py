"""CPU: hp_rgb_to_yuv_host, hp_yuv_forward_coefficients and hp_yuv_padded_size against tests/to_yuv_ref.py (the rule of DESIGN.md 1.1 "Encoder
hand-off" restated in numpy): coefficients, every layout pair byte for byte with the untouched row padding, padding by edge replication, grey frames,
the distance to the float rule of hp_yuv_colours, the round trip through hp_resize_yuv's formulas, and every refusal."""
import ctypes as C

import numpy as np
import pytest

import to_yuv_ref as ref
from hyperpose_amd import _lib, frontend
from hyperpose_amd._lib import HP_ERR_INVALID, HP_OK, RgbImage, YuvImage
from overlay_ref import RGB as SKELETON_RGB

# src (w, h) -> dst (w, h); None: the smallest size the layout holds
SIZES = [((1, 1), None), ((2, 2), (2, 2)), ((3, 5), (4, 6)), ((31, 3), (32, 4)), ((30, 20), "align16")]
PITCH = 5  # odd: host planes follow no alignment rule


def dst_size(fmt, src, dst):
    if dst is None:
        return ref.padded_size(fmt, *src)
    if dst == "align16":
        size = frontend.yuv_padded_size(fmt, *src, 16)
        assert size == (32, 32)
        return size
    return dst


def sizes_of(fmt):
    return SIZES + ([((3, 5), (3, 5))] if fmt == "i444" else [])


def frames_of(fmt_rgb, w, h, seed):
    return [ref.random_frame(seed, fmt_rgb, w, h), ref.extremes_frame(fmt_rgb, w, h)]


def assert_same(planes, backs, what):
    for k, (p, b) in enumerate(zip(planes, backs)):
        assert np.array_equal(p.base, b), f"{what}: plane {k} differs (padding included)"


# ---- coefficients ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("rng", ref.RANGES)
@pytest.mark.parametrize("matrix", ref.MATRICES)
def test_forward_coefficients_equal_the_ref(matrix, rng, depth):
    k = frontend.yuv_forward_coefficients(matrix, rng, depth)
    assert k == ref.coefficients(matrix, rng, depth)
    assert sum(k[5:8]) == 0 and sum(k[8:11]) == 0


def test_forward_coefficients_bt601_limited_8():
    assert frontend.yuv_forward_coefficients("bt601", "limited", 8) == [16, 128, 67315, 132155, 25665, -38856, -76282, 115138, 115138, -96414, -18724]


def test_forward_coefficients_refusals():
    out = (C.c_int32 * 11)()
    for args, word in (((3, 0, 8), "matrix"), ((0, 2, 8), "range"), ((0, 0, 9), "depth")):
        assert _lib.lib().hp_yuv_forward_coefficients(*args, out) == HP_ERR_INVALID
        assert word in _lib.lib().hp_last_error().decode()


def test_padded_size():
    for fmt in ref.YUV_FORMATS:
        for w, h, align in ((1, 1, 1), (3, 5, 1), (30, 20, 16), (1920, 1080, 16), (322, 182, 3), (7, 9, 256), (8192, 8192, 1)):
            assert frontend.yuv_padded_size(fmt, w, h, align) == ref.padded_size(fmt, w, h, align)
    assert frontend.yuv_padded_size("nv12", 1920, 1080, 16) == (1920, 1088)
    assert frontend.yuv_padded_size("i444", 3, 5, 1) == (3, 5)
    pw, ph = C.c_int(), C.c_int()
    for args, word in (((0, 4, 4, 0), "align 0"), ((0, 4, 4, 257), "align 257"), ((9, 4, 4, 2), "format 9"), ((0, 0, 4, 2), "0 x 4")):
        assert _lib.lib().hp_yuv_padded_size(*args, C.byref(pw), C.byref(ph)) == HP_ERR_INVALID
        assert word in _lib.lib().hp_last_error().decode()


# ---- the host twin against the ref, byte for byte ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ref.YUV_FORMATS)
def test_every_layout_pair_bt709_limited(fmt):
    for n, fmt_rgb in enumerate(ref.RGB_FORMATS):
        for src, dst in sizes_of(fmt):
            size = dst_size(fmt, src, dst)
            for frame in frames_of(fmt_rgb, *src, seed=100 + n):
                got = frontend.rgb_to_yuv_host(frame, fmt_rgb, fmt, "bt709", "limited", pad_to=size, pitch=PITCH)
                _, want = ref.convert(frame, fmt_rgb, fmt, "bt709", "limited", size, PITCH)
                assert_same(got, want, f"{fmt_rgb} {src} -> {fmt} {size}")


@pytest.mark.parametrize("rng", ref.RANGES)
@pytest.mark.parametrize("matrix", ref.MATRICES)
@pytest.mark.parametrize("fmt", ["nv12", "p010", "i444"])
def test_every_matrix_and_range_from_bgra(fmt, matrix, rng):
    for src, dst in sizes_of(fmt):
        size = dst_size(fmt, src, dst)
        for frame in frames_of("bgra", *src, seed=7):
            got = frontend.rgb_to_yuv_host(frame, "bgra", fmt, matrix, rng, pad_to=size, pitch=PITCH)
            _, want = ref.convert(frame, "bgra", fmt, matrix, rng, size, PITCH)
            assert_same(got, want, f"bgra {src} -> {fmt} {size} {matrix} {rng}")


def test_a_pitched_source_is_read_inside_its_rows():
    back = np.full((5, 3 * 4 + 8), 0xEE, np.uint8)
    view = back[:, :12].reshape(5, 3, 4)
    view[...] = ref.random_frame(3, "rgba", 3, 5)
    got = frontend.rgb_to_yuv_host(view, "rgba", "i420", pad_to=(4, 6), pitch=PITCH)
    _, want = ref.convert(view, "rgba", "i420", size=(4, 6), pitch=PITCH)
    assert_same(got, want, "pitched rgba")


# ---- properties ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", ref.RANGES)
@pytest.mark.parametrize("matrix", ref.MATRICES)
def test_grey_frames_have_neutral_chroma(matrix, rng):
    grey = ref.random_frame(5, "gray", 31, 3)
    bgra = np.stack([grey, grey, grey, ref.random_frame(6, "gray", 31, 3)], axis=-1)
    for fmt in ("nv12", "p010", "i444", "yuy2"):
        _, _, depth, shift = ref.LAYOUT[fmt]
        c_off = frontend.yuv_forward_coefficients(matrix, rng, depth)[1]
        for frame, fmt_rgb in ((grey, "gray"), (bgra, "bgra")):
            _, U, V = ref.sample_views(frontend.rgb_to_yuv_host(frame, fmt_rgb, fmt, matrix, rng, pad_to=(32, 4)), fmt)
            assert np.all(U >> shift == c_off) and np.all(V >> shift == c_off)


@pytest.mark.parametrize("fmt", ref.YUV_FORMATS)
def test_padding_is_edge_replication(fmt):
    for fmt_rgb in ("bgr24", "argb", "gray"):
        frame = ref.random_frame(11, fmt_rgb, 31, 3)
        W, H = 48, 16
        padded = frame[np.minimum(np.arange(H), 2)][:, np.minimum(np.arange(W), 30)]
        a = frontend.rgb_to_yuv_host(frame, fmt_rgb, fmt, pad_to=(W, H))
        b = frontend.rgb_to_yuv_host(np.ascontiguousarray(padded), fmt_rgb, fmt, pad_to=(W, H))
        for p, q in zip(a, b):
            assert np.array_equal(p, q)


@pytest.mark.parametrize("rng", ref.RANGES)
@pytest.mark.parametrize("matrix", ref.MATRICES)
def test_skeleton_colours_within_one_of_the_float_rule(matrix, rng):
    """The bound the rule was checked against over all 2^24 colours: at most 1 code value from hp_yuv_colours (float64, nearbyint).  8 bits through 1 x 1
    I444 frames; 10 bits through 2 x 2 P010 frames of one colour, whose box mean is the colour itself."""
    for depth, fmt, n in ((8, "i444", 1), (10, "p010", 2)):
        want = frontend.yuv_colours(matrix, rng, depth)
        shift = ref.LAYOUT[fmt][3]
        for i, (r, g, b) in enumerate(SKELETON_RGB):
            frame = np.tile(np.array([r, g, b], np.uint8), (n, n, 1))
            Y, U, V = ref.sample_views(frontend.rgb_to_yuv_host(frame, "rgb24", fmt, matrix, rng), fmt)
            got = np.array([Y[0, 0], U[0, 0], V[0, 0]], np.int64) >> shift
            assert np.abs(got - want[i]).max() <= 1, (depth, i, got, want[i])


def test_round_trip_for_the_record(capsys):
    """hp_rgb_to_yuv_host, then the decode hp_yuv_coefficients documents: the largest absolute error per (matrix, range, depth), printed (DESIGN.md 1.1
    quotes the figures).  Asserted: the library's bytes give the figure the ref's bytes give.  8 bits: I444; 10 bits: P010 on a picture whose 2 x 2
    blocks hold one colour each, so that sub-sampling loses nothing."""
    r = np.random.default_rng(42)
    small = r.integers(0, 256, (32, 48, 3), dtype=np.uint8)
    small[0, :8] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255]]
    figures = {}
    for depth, fmt, frame in ((8, "i444", small), (10, "p010", small.repeat(2, axis=0).repeat(2, axis=1))):
        shift = ref.LAYOUT[fmt][3]
        for matrix in ref.MATRICES:
            for rng in ref.RANGES:
                errs = []
                for planes in (frontend.rgb_to_yuv_host(frame, "rgb24", fmt, matrix, rng), ref.convert(frame, "rgb24", fmt, matrix, rng)[0]):
                    Y, U, V = (a.astype(np.int64) >> shift for a in ref.sample_views(planes, fmt))
                    if fmt == "p010":
                        U, V = U.repeat(2, axis=0).repeat(2, axis=1), V.repeat(2, axis=0).repeat(2, axis=1)
                    B, G, R = ref.decode444(Y, U, V, matrix, rng, depth)
                    errs.append(int(np.abs(np.stack([R, G, B], axis=-1) - frame.astype(np.int64)).max()))
                assert errs[0] == errs[1]
                figures[(matrix, rng, depth)] = errs[0]
    with capsys.disabled():
        print("\nround trip, max |error| in 8-bit code values:", ", ".join(f"{m} {g} {d}-bit: {e}" for (m, g, d), e in figures.items()))


# ---- refusals: HP_ERR_INVALID, the message names the layout and the quantity, dst untouched ------------------------------------------------------------

def _call(src, dst):
    rc = _lib.lib().hp_rgb_to_yuv_host(C.byref(src), C.byref(dst))
    return rc, _lib.lib().hp_last_error().decode()


def _valid(fmt="nv12", fmt_rgb="bgra", sw=6, sh=4, dw=8, dh=4):
    frame = ref.random_frame(1, fmt_rgb, sw, sh)
    src, keep = frontend.rgb_host_image(frame, fmt_rgb)
    planes, backs = ref.blank_planes(fmt, dw, dh, pitch=4)
    dst = frontend.yuv_image(fmt, [p.ctypes.data for p in planes], [p.strides[0] for p in planes], dw, dh, "bt709", "limited")
    return src, dst, backs, keep


def test_the_valid_call_of_the_refusal_tests_passes():
    src, dst, backs, _ = _valid()
    assert _call(src, dst)[0] == HP_OK
    assert any(np.any(b != 0xA5) for b in backs)


REFUSALS = [
    ("dst format", lambda s, d: setattr(d, "format", 9), ["unknown format 9"]),
    ("dst matrix", lambda s, d: setattr(d, "matrix", 3), ["HP_YUV_NV12", "matrix 3"]),
    ("dst range", lambda s, d: setattr(d, "range", 2), ["HP_YUV_NV12", "range 2"]),
    ("dst odd height", lambda s, d: setattr(d, "height", 5), ["HP_YUV_NV12", "even", "8 x 5"]),
    ("dst empty", lambda s, d: setattr(d, "width", 0), ["HP_YUV_NV12", "0 x 4"]),
    ("dst null plane", lambda s, d: d.plane.__setitem__(1, None), ["HP_YUV_NV12", "plane 1 is null"]),
    ("dst short stride", lambda s, d: d.stride.__setitem__(0, 7), ["HP_YUV_NV12", "stride 7", "plane 0"]),
    ("src format", lambda s, d: setattr(s, "format", 7), ["unknown format 7"]),
    ("src null", lambda s, d: setattr(s, "data", None), ["HP_RGB_BGRA32", "data is null"]),
    ("src empty", lambda s, d: setattr(s, "height", 0), ["HP_RGB_BGRA32", "6 x 0"]),
    ("src short stride", lambda s, d: setattr(s, "stride", 23), ["HP_RGB_BGRA32", "stride 23"]),
    ("dst narrower", lambda s, d: setattr(s, "width", 10) or setattr(s, "stride", 64), ["HP_YUV_NV12", "width 8", "HP_RGB_BGRA32", "10"]),
    ("dst lower", lambda s, d: setattr(s, "height", 6), ["HP_YUV_NV12", "height 4", "HP_RGB_BGRA32", "6"]),
]


@pytest.mark.parametrize("name,spoil,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, spoil, words):
    src, dst, backs, _ = _valid()
    spoil(src, dst)
    rc, msg = _call(src, dst)
    assert rc == HP_ERR_INVALID, msg
    assert msg.startswith("hp_rgb_to_yuv_host: ")
    for w in words:
        assert w in msg, msg
    assert all(np.all(b == 0xA5) for b in backs)


@pytest.mark.parametrize("w,h", [(8194, 2), (2, 8194)])
def test_an_output_over_8192_is_refused(w, h):
    src, dst, backs, _ = _valid(sw=1, sh=1, dw=w, dh=h)
    rc, msg = _call(src, dst)
    assert rc == HP_ERR_INVALID and "HP_YUV_NV12" in msg and f"{w} x {h}" in msg and "8192" in msg
    assert all(np.all(b == 0xA5) for b in backs)


def test_null_descriptions_are_refused():
    src, dst, _, _ = _valid()
    assert _lib.lib().hp_rgb_to_yuv_host(None, C.byref(dst)) == HP_ERR_INVALID
    assert _lib.lib().hp_rgb_to_yuv_host(C.byref(src), None) == HP_ERR_INVALID
    assert isinstance(src, RgbImage) and isinstance(dst, YuvImage)
