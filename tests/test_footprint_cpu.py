"""CPU: the write-footprint checker (tests/footprint.py) on synthetic raw buffers - no library call.  Odd H with P = 1, so that the fp32
layout has its separator row; C = 19, so that the first pad channel lies directly behind the data inside one 4-channel vector."""
import numpy as np
import pytest

import footprint as F

H, W, C, P, NB = 5, 6, 19, 1, 3
DTYPES = [np.float16, np.float32]


def _raw(dtype, seed=0):
    g = F.make_geom(H, W, C, P, NB, f32=dtype == np.float32)
    a = np.zeros(F.raw_shape(g), dtype)
    a[F.interior_mask(g)] = np.random.default_rng(seed).normal(size=NB * H * W * C).astype(dtype)
    return a, g


def test_geometry_and_mask():
    g16, g32 = F.make_geom(H, W, C, P, NB, False), F.make_geom(H, W, C, P, NB, True)
    assert g16["rows"] == 7 and g32["rows"] == 8 and g16["cs"] == g32["cs"] == 32
    assert F.make_geom(H, W, C, 0, NB, True)["rows"] == H      # no halo: no separator row either
    assert F.make_geom(4, W, C, 1, NB, True)["rows"] == 6
    for g in (g16, g32):
        m = F.interior_mask(g)
        assert m.shape == (NB, g["rows"], W + 2, 32) and m.sum() == NB * H * W * C
        assert m[NB - 1, P, P, 0] and m[0, P + H - 1, P + W - 1, C - 1]
        assert not m[0, 0].any() and not m[0, P + H:].any() and not m[0, :, 0].any() and not m[0, :, P + W:].any() and not m[..., C:].any()
    assert F.region_of(g32, 7, 3, 0) == "separator row" and F.region_of(g32, 6, 3, 0) == "bottom halo"


# (region, y, x, c); the separator row exists in the fp32 layout only
PLANTS = [("top halo", 0, 3, 2), ("bottom halo", P + H, 3, 2), ("left halo", 3, 0, 2), ("right halo", 3, P + W, 2),
          ("pad channel", 3, 3, 31), ("pad channel", 3, 3, C)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("region,y,x,c", PLANTS)
def test_planted_value_is_found_and_named(dtype, region, y, x, c):
    a, g = _raw(dtype)
    assert C % 4 != 0
    a[1, y, x, c] = 0.5
    with pytest.raises(AssertionError) as ei:
        F.check_zero_outside(a, g, "tensor 7")
    msg = str(ei.value)
    assert "tensor 7" in msg and f"frame 1 (y={y}, x={x}, c={c}) = 0.5 [{region}]" in msg and f"regions: {region};" in msg


def test_planted_value_in_the_separator_row():
    a, g = _raw(np.float32)
    assert g["rows"] == H + 2 * P + 1
    a[2, g["rows"] - 1, 3, 0] = -3.0
    with pytest.raises(AssertionError, match=r"frame 2 \(y=7, x=3, c=0\) = -3.0 \[separator row\]"):
        F.check_zero_outside(a, g)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_value_is_found(dtype, value):
    a, g = _raw(dtype)
    a[0, 2, P + W, 1] = value
    with pytest.raises(AssertionError, match="right halo"):
        F.check_zero_outside(a, g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_untouched_and_signed_zero_pass(dtype):
    a, g = _raw(dtype)
    F.check_zero_outside(a, g)
    a[~F.interior_mask(g)] = -0.0
    assert np.signbit(a[0, 0, 0, 0])
    F.check_zero_outside(a, g)
    a[F.interior_mask(g)] = np.nan      # what the interior holds is not this check's business
    F.check_zero_outside(a, g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_changed_byte_in_a_later_frame(dtype):
    a, g = _raw(dtype)
    n = 1
    for first in (0, 1):                 # the snapshot holds frames first .. : the whole buffer, or frames n .. only
        before = a[first:].copy()
        b = a.copy()
        b[0] += 1                        # frames < n may change
        F.check_frames_unchanged(before, first, b, n)
        raw = b.view(np.uint8)
        flat = np.ravel_multi_index((2, 0, 0, 5), a.shape) * a.dtype.itemsize   # a halo element of frame 2: one low byte flips
        raw.reshape(-1)[flat] ^= 1
        with pytest.raises(AssertionError, match=r"changed 1 element\(s\) of frames 1\.\.2; first: frame 2 \(y=0, x=0, c=5\)"):
            F.check_frames_unchanged(before, first, b, n, "tensor 3")
    # bitwise, not numeric: -0.0 for 0.0 is a change here
    b = a.copy()
    b[1, 0, 0, 0] = -0.0
    with pytest.raises(AssertionError, match="frame 1"):
        F.check_frames_unchanged(a, 0, b, n)
    F.check_zero_outside(b, g)
    with pytest.raises(AssertionError):  # a snapshot that cannot hold frames `first` .. of this buffer
        F.check_frames_unchanged(a[1:], 0, a, n)
