"""The rule of hp_rgb_image (include/hp_hip.h, "packed RGB and grey frames") a second time, in numpy: memory order is as the name reads, the fourth
byte is ignored, grey gives B = G = R.  Written from the header's text, not from hyperpose_amd/csrc/rgb_formats.hpp or _lib.RGB_LAYOUTS."""
import numpy as np

# name -> the channels of a pixel in memory order ("X": the ignored fourth byte, "Y": the grey sample)
ORDER = {"bgr24": "BGR", "rgb24": "RGB", "bgra": "BGRX", "rgba": "RGBX", "argb": "XRGB", "abgr": "XBGR", "gray": "Y"}
FORMATS = list(ORDER)
COLOUR = [f for f in FORMATS if f != "gray"]


def pixel_bytes(fmt):
    return len(ORDER[fmt])


def to_bgr(arr, fmt):
    """[h, w, n] (or [h, w] for grey) uint8 in the layout's memory order -> [h, w, 3] BGR."""
    arr = np.asarray(arr)
    o = ORDER[fmt]
    if o == "Y":
        assert arr.ndim == 2
        return np.stack([arr, arr, arr], axis=-1).astype(np.uint8)
    assert arr.ndim == 3 and arr.shape[2] == len(o)
    return np.stack([arr[..., o.index(c)] for c in "BGR"], axis=-1).astype(np.uint8)


def from_bgr(bgr, fmt, rng):
    """A frame of layout ``fmt`` whose to_bgr is ``bgr`` (grey: the frame is the B channel, so pass a picture with B = G = R for an exact twin).  The
    fourth byte is random and holds 0 and 255 somewhere (whenever the frame has two pixels): a kernel that reads, multiplies or blends alpha fails."""
    bgr = np.asarray(bgr, np.uint8)
    o = ORDER[fmt]
    if o == "Y":
        return np.ascontiguousarray(bgr[..., 0])
    h, w, _ = bgr.shape
    out = np.empty((h, w, len(o)), np.uint8)
    for k, c in enumerate(o):
        if c == "X":
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            a.flat[0] = 0
            a.flat[-1] = 255 if a.size > 1 else a.flat[-1]
            a[rng.random((h, w)) < 0.2] = 0
            a.flat[-1] = 255 if a.size > 1 else a.flat[-1]
            out[..., k] = a
        else:
            out[..., k] = bgr[..., "BGR".index(c)]
    return out


def padded(arr, extra, fill):
    """``arr`` as a view into rows that are ``extra`` bytes longer, the padding poisoned with ``fill``: (view, the whole 2-D byte buffer)."""
    arr = np.ascontiguousarray(arr, np.uint8)
    h, w = arr.shape[:2]
    row = arr.size // h
    buf = np.full((h, row + extra), fill, np.uint8)
    buf[:, :row] = arr.reshape(h, row)
    return buf[:, :row].reshape(arr.shape), buf
