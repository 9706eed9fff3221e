"""The tests' own statement of the map view's picture (hp_mapview_*, include/hp_hip.h; DESIGN.md 1.1 "Map view"), written from the rules and calling
the library for nothing it checks: the index plane in numpy float32, the taps in Python floats (doubles), everything after them in int64 arrays, the
palettes in float64.  Shared by tests/test_mapview_host.py, tests/test_mapview_gpu.py, tests/test_mapview_engine_gpu.py and tools/mapview_bench.py."""
import math

import numpy as np
from overlay_ref import K, LAYOUT, random_frame, sample_views  # noqa: F401  (re-exported for the tests)

f32 = np.float32
ONE = 2048


def axes(code):
    """(swap, flip_x, flip_y) of an HP_ORIENT_* code = q + 4 * m"""
    q, m = code & 3, (code >> 2) & 1
    return q & 1, ((q >> 1) & 1) ^ m, (q ^ (q >> 1)) & 1


def channels_of(C, mode, channels=None):
    if channels is not None:
        return tuple(channels)
    return (0, C // 2, 2) if mode == "field" else (0, C, 1)


def index_plane(maps, mode="max", channels=None, gain=1.0):
    """rule 1: maps float32 [C, mh, mw] -> int64 [mh, mw] in [0, 255]"""
    maps = np.asarray(maps, f32)
    c0, cn, step = channels_of(maps.shape[0], mode, channels)
    with np.errstate(all="ignore"):
        m = np.zeros(maps.shape[1:], f32)
        for k in range(cn):
            c = c0 + k * step
            if mode == "max":
                v = maps[c]
            else:
                v = (maps[c] * maps[c]).astype(f32) + (maps[c + 1] * maps[c + 1]).astype(f32)
            m = np.where(v > m, v, m).astype(f32)
        if mode != "max":
            m = np.sqrt(m).astype(f32)
        t = (m * f32(gain)).astype(f32)
        t = np.where(t < f32(1), t, f32(1)).astype(f32)
        return np.rint((t * f32(255)).astype(f32)).astype(np.int64)


def taps(U, m, cover=1.0):
    """rule 2: [(i0, i1, weight)] per upright pixel, Python floats"""
    out = []
    scale = (float(cover) * m) / U
    for u in range(U):
        s = (u + 0.5) * scale - 0.5
        if s < 0:
            out.append((0, 0, 0))
            continue
        i = math.floor(s)
        out.append((min(i, m - 1), min(i + 1, m - 1), int(np.rint((s - i) * 2048.0))))
    return out


def letterbox_cover(frame_w, frame_h, in_w, in_h):
    """the cover of a letter-boxed slot: the inner size the front end's letterbox gives (hp_letterbox_inner, which has tests of its own and is
    not what these tests check) over the input size"""
    from hyperpose_amd import frontend
    iw, ih = frontend.letterbox_inner(frame_w, frame_h, in_w, in_h)
    return iw / float(in_w), ih / float(in_h)


def index_map(plane, w, h, orientation=0, cover=(1.0, 1.0)):
    """rules 3 and 4: int64 [h, w], the index of every stored pixel of a w x h roi"""
    mh, mw = plane.shape
    swap, fx, fy = axes(orientation)
    tx = np.array(taps(h if swap else w, mw, cover[0]), np.int64)
    ty = np.array(taps(w if swap else h, mh, cover[1]), np.int64)
    ly, lx = np.mgrid[0:h, 0:w]
    a = w - 1 - lx if fx else lx
    b = h - 1 - ly if fy else ly
    ux, uy = (b, a) if swap else (a, b)
    x0, x1, wx = tx[ux, 0], tx[ux, 1], tx[ux, 2]
    y0, y1, wy = ty[uy, 0], ty[uy, 1], ty[uy, 2]
    p = plane.astype(np.int64)
    top = p[y0, x0] * (ONE - wx) + p[y0, x1] * wx
    bot = p[y1, x0] * (ONE - wx) + p[y1, x1] * wx
    assert top.max() < 2 ** 31
    total = top * (ONE - wy) + bot * wy + (1 << 21)
    assert total.max() < 2 ** 31
    idx = total >> 22
    assert idx.min() >= 0 and idx.max() <= 255
    return idx


def palette(kind="jet", alpha="constant"):
    """rule 5: int64 [256, 4] (R, G, B, A), float64 formulas"""
    out = []
    clamp = lambda c: min(1.0, max(0.0, c))  # noqa: E731
    for i in range(256):
        t = i / 255.0
        if kind == "jet":
            rgb = (clamp(1.5 - abs(4 * t - 3)), clamp(1.5 - abs(4 * t - 2)), clamp(1.5 - abs(4 * t - 1)))
        elif kind == "heat":
            rgb = (clamp(3 * t), clamp(3 * t - 1), clamp(3 * t - 2))
        else:
            rgb = (t, t, t)
        out.append([int(np.rint(255.0 * c)) for c in rgb] + [i if alpha == "scaled" else 255])
    return np.array(out, np.int64)


def yuv_of(rgb, matrix, rng, depth):
    """(Y, U, V) at `depth` bits of one (R, G, B) in [0, 255]: hp_yuv_colours' formulas in float64"""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    top, up, half = float((1 << depth) - 1), float(1 << (depth - 8)), float(1 << (depth - 1))
    r, g, b = (c / 255.0 for c in rgb)
    y = kr * r + kg * g + kb * b
    cb, cr = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
    if rng == "limited":
        v = [(16.0 + 219.0 * y) * up, (128.0 + 224.0 * cb) * up, (128.0 + 224.0 * cr) * up]
    else:
        v = [y * top, half + cb * top, half + cr * top]
    return [int(min(top, max(0.0, np.rint(c)))) for c in v]


def palette_yuv(rgba, matrix, rng, depth):
    return np.array([yuv_of([int(v) for v in e[:3]], matrix, rng, depth) + [int(e[3])] for e in rgba], np.int64)


def weight(opacity):
    return int(np.rint(np.float64(np.float32(opacity)) * 256.0))


def _mix(view, idx, colour, wts, depth, shift):
    """view (a numpy view of the samples that idx addresses; idx < 0: no index) <- rule 6"""
    safe = np.maximum(idx, 0)
    w = np.where(idx >= 0, wts[safe], 0)
    old = (view.astype(np.int64) >> shift) & ((1 << depth) - 1)
    new = (colour[safe] * w + old * (256 - w) + 128) >> 8
    mask = w > 0
    view[mask] = (new[mask] << shift).astype(view.dtype)


def paint(frame, maps, fmt=None, matrix="bt601", rng="limited", mode="max", pal=None, opacity=0.5, gain=1.0, channels=None, cover=(1.0, 1.0),
          orientation=0, roi=None):
    """Blend in place: `frame` is uint8 [h, w, 3] BGR (fmt None) or the list of 2-D plane arrays of layout `fmt`; `maps` float32 [C, mh, mw] of the
    frame; `pal` int [256, 4] (R, G, B, A).  Returns the index plane."""
    pal = palette() if pal is None else np.asarray(pal, np.int64)
    plane = index_plane(maps, mode, channels, gain)
    wts = (weight(opacity) * pal[:, 3] + 127) // 255
    if fmt is None:
        H, W = frame.shape[:2]
        rx, ry, rw, rh = roi or (0, 0, W, H)
        idx = index_map(plane, rw, rh, orientation, cover)
        for c in range(3):
            _mix(frame[ry:ry + rh, rx:rx + rw, c], idx, pal[:, 2 - c], wts, 8, 0)
        return plane
    sx, sy, depth, shift = LAYOUT[fmt]
    Y, U, V = sample_views(frame, fmt)
    H, W = Y.shape
    rx, ry, rw, rh = roi or (0, 0, W, H)
    idx = index_map(plane, rw, rh, orientation, cover)
    table = palette_yuv(pal, matrix, rng, depth)
    _mix(Y[ry:ry + rh, rx:rx + rw], idx, table[:, 0], wts, depth, shift)
    full = np.full((H, W), -1, np.int64)
    full[ry:ry + rh, rx:rx + rw] = idx
    best = full.reshape(H >> sy, 1 << sy, W >> sx, 1 << sx).max(axis=(1, 3))  # the largest index over a chroma sample's pixels inside the roi
    _mix(U, best, table[:, 1], wts, depth, shift)
    _mix(V, best, table[:, 2], wts, depth, shift)
    return plane


def blob_maps(seed, frames, C, mh, mw):
    """float32 [frames, C, mh, mw]: per channel a few smooth blobs of either sign on small noise, peaks a little above 1, every frame different"""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:mh, 0:mw].astype(np.float64)
    out = r.normal(0.0, 0.03, (frames, C, mh, mw))
    for f in range(frames):
        for c in range(C):
            for _ in range(2):
                cx, cy, s = r.uniform(0, mw), r.uniform(0, mh), r.uniform(0.6, 2.0)
                out[f, c] += r.uniform(-0.5, 1.2) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
    return out.astype(f32)
