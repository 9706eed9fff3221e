"""The rule of hp_rgb_to_yuv (DESIGN.md 1.1 "Encoder hand-off") restated in numpy and Python integers: coefficients from float64, the pixel and chroma
formulas, edge-replication padding, and where samples lie - the planes' geometry through hp_yuv_plane_layout (frontend.yuv_plane_shapes), the order
inside them from the layouts' names.  Nothing here is copied from hyperpose_amd/csrc/to_yuv.hpp; the tests compare the library against this."""
import numpy as np

S = 18
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MATRICES, RANGES = list(K), ["limited", "full"]
# layout -> (chroma shift x, chroma shift y, depth, left shift of a stored sample)
LAYOUT = {"nv12": (1, 1, 8, 0), "i420": (1, 1, 8, 0), "p010": (1, 1, 10, 6), "i010": (1, 1, 10, 0), "nv16": (1, 0, 8, 0), "i422": (1, 0, 8, 0),
          "yuy2": (1, 0, 8, 0), "uyvy": (1, 0, 8, 0), "i444": (0, 0, 8, 0)}
YUV_FORMATS = list(LAYOUT)
# layout -> (bytes per pixel, byte offsets of R, G, B): memory order is as the name reads, grey gives R = G = B
RGB = {"bgr24": (3, 2, 1, 0), "rgb24": (3, 0, 1, 2), "bgra": (4, 2, 1, 0), "rgba": (4, 0, 1, 2), "argb": (4, 1, 2, 3), "abgr": (4, 3, 2, 1),
       "gray": (1, 0, 0, 0)}
RGB_FORMATS = list(RGB)


def coefficients(matrix, rng, depth):
    """[y_off, c_off, YR, YG, YB, UR, UG, UB, VR, VG, VB]"""
    kr, kb = K[matrix]
    one, up = float(1 << S), float(1 << (depth - 8))
    if rng == "limited":
        ys, cs, y_off, c_off = 219.0 * up / 255.0, 224.0 * up / 255.0, 16 << (depth - 8), 128 << (depth - 8)
    else:
        ys = cs = ((1 << depth) - 1) / 255.0
        y_off, c_off = 0, 1 << (depth - 1)
    rint = lambda v: int(np.rint(v))  # noqa: E731  (round half to even, as C's rint in the default mode)
    YR, YB = rint(kr * ys * one), rint(kb * ys * one)
    YG = rint(ys * one) - YR - YB
    UB, UR = rint(0.5 * cs * one), -rint(kr / (2.0 * (1.0 - kb)) * cs * one)
    UG = -UB - UR
    VR, VB = rint(0.5 * cs * one), -rint(kb / (2.0 * (1.0 - kr)) * cs * one)
    VG = -VR - VB
    return [y_off, c_off, YR, YG, YB, UR, UG, UB, VR, VG, VB]


def padded_size(fmt, w, h, align=1):
    from math import lcm
    sx, sy, _, _ = LAYOUT[fmt]
    ax, ay = lcm(align, 1 << sx), lcm(align, 1 << sy)
    return -(-w // ax) * ax, -(-h // ay) * ay


def rgb_of(frame, fmt_rgb):
    """int64 [h, w, 3] (R, G, B) of a host frame [h, w, pixel bytes] (grey: [h, w])"""
    pb, r, g, b = RGB[fmt_rgb]
    a = np.asarray(frame).astype(np.int64)
    if pb == 1:
        return np.stack([a, a, a], axis=-1)
    return np.stack([a[..., r], a[..., g], a[..., b]], axis=-1)


def pad_edges(rgb, w, h):
    """[h, w, 3]: pixel (x, y) is rgb[min(y, sh - 1), min(x, sw - 1)]"""
    sh, sw = rgb.shape[:2]
    return rgb[np.minimum(np.arange(h), sh - 1)][:, np.minimum(np.arange(w), sw - 1)]


def samples(rgb, fmt, matrix, rng):
    """(Y [h, w], U, V [h >> sy, w >> sx]) code values, int64, of an (already padded) int64 [h, w, 3] (R, G, B) picture"""
    sx, sy, depth, _ = LAYOUT[fmt]
    k = coefficients(matrix, rng, depth)
    top = (1 << depth) - 1
    R, G, B = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    Y = np.clip((k[2] * R + k[3] * G + k[4] * B + (k[0] << S) + (1 << (S - 1))) >> S, 0, top)
    h, w = R.shape
    box = lambda a: a.reshape(h >> sy, 1 << sy, w >> sx, 1 << sx).sum(axis=(1, 3))  # noqa: E731
    Rs, Gs, Bs = box(R), box(G), box(B)
    log2n = sx + sy
    bias = ((k[1] << S) + (1 << (S - 1))) << log2n
    U = np.clip((k[5] * Rs + k[6] * Gs + k[7] * Bs + bias) >> (S + log2n), 0, top)
    V = np.clip((k[8] * Rs + k[9] * Gs + k[10] * Bs + bias) >> (S + log2n), 0, top)
    return Y, U, V


def sample_views(planes, fmt):
    """(Y, U, V) as numpy views into the planes: the layouts, restated from their names"""
    if fmt in ("yuy2", "uyvy"):
        p = planes[0]
        return (p[:, 0::2], p[:, 1::4], p[:, 3::4]) if fmt == "yuy2" else (p[:, 1::2], p[:, 0::4], p[:, 2::4])
    if fmt in ("nv12", "nv16", "p010"):
        return planes[0], planes[1][:, 0::2], planes[1][:, 1::2]
    return planes[0], planes[1], planes[2]


def blank_planes(fmt, w, h, pitch=0, fill=0xA5):
    """(plane views, backing byte arrays): planes of a w x h frame whose rows are `pitch` bytes longer than the picture's, every byte `fill`"""
    from hyperpose_amd import frontend
    dt = np.dtype(np.uint16 if LAYOUT[fmt][2] == 10 else np.uint8)
    views, backs = [], []
    for rows, cols in frontend.yuv_plane_shapes(fmt, w, h):
        stride = cols * dt.itemsize + pitch
        back = np.full((rows, stride), fill, np.uint8)
        views.append(np.ndarray((rows, cols), dt, buffer=back, strides=(stride, dt.itemsize)))
        backs.append(back)
    return views, backs


def convert(frame, fmt_rgb, fmt, matrix="bt709", rng="limited", size=None, pitch=0, fill=0xA5):
    """(plane views, backing arrays) of the converted frame; `size` (w, h) pads by edge replication (None: the smallest size the layout holds)"""
    rgb = rgb_of(frame, fmt_rgb)
    w, h = size or padded_size(fmt, rgb.shape[1], rgb.shape[0])
    Y, U, V = samples(pad_edges(rgb, w, h), fmt, matrix, rng)
    views, backs = blank_planes(fmt, w, h, pitch, fill)
    shift = LAYOUT[fmt][3]
    for view, val in zip(sample_views(views, fmt), (Y, U, V)):
        view[...] = (val << shift).astype(view.dtype)
    return views, backs


def random_frame(seed, fmt_rgb, w, h):
    pb = RGB[fmt_rgb][0]
    r = np.random.default_rng(seed)
    return r.integers(0, 256, (h, w) if pb == 1 else (h, w, pb), dtype=np.uint8)


def extremes_frame(fmt_rgb, w, h):
    """0 / 255 corners, pure primaries and their complements in between, cycling; a fourth byte alternates 0 / 255"""
    pb, r, g, b = RGB[fmt_rgb]
    cols = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    idx = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :]) % len(cols)
    idx[0, 0], idx[0, -1], idx[-1, 0], idx[-1, -1] = 0, 1, 1, 0
    rgb = np.array(cols, np.uint8)[idx]
    if pb == 1:
        return rgb[..., 0].copy()
    out = np.zeros((h, w, pb), np.uint8)
    if pb == 4:
        out[...] = ((np.arange(w) % 2) * 255).astype(np.uint8)[None, :, None]
    out[..., r], out[..., g], out[..., b] = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return out


def decode444(Y, U, V, matrix, rng, depth=8):
    """8-bit (B, G, R) of 4:4:4 samples by the formulas hp_yuv_coefficients documents (include/hp_hip.h), k its table"""
    from hyperpose_amd import frontend
    k = frontend.yuv_coefficients(matrix, rng, depth)
    Y, u, v = Y.astype(np.int64), U.astype(np.int64) - k[1], V.astype(np.int64) - k[1]
    yy = np.maximum(0, Y - k[0]) * k[2] + (1 << 19)
    sat = lambda a: np.clip(a, 0, 255)  # noqa: E731
    return sat((yy + k[3] * u) >> 20), sat((yy + k[5] * v + k[4] * u) >> 20), sat((yy + k[6] * v) >> 20)
