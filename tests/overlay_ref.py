"""The tests' own statement of the overlay picture (hp_overlay_*, include/hp_hip.h): a numpy painter that calls the library for
nothing it checks.  The primitive list is restated in numpy float32, the coverage rules use Python integers (no width to overflow), one
primitive at a time over its own bounding box, the colour tables are float64, and the samples are written through numpy views of the planes.
Shared by tests/test_overlay_host.py, tests/test_overlay_gpu.py and tests/test_cli_overlay.py; coverage maps are computed once per case."""
import functools

import numpy as np

from hyperpose_amd._lib import HUMAN_DTYPE

PAIRS = [(1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16), (0, 15),
         (15, 17), (2, 16), (5, 17)]
RGB = [(255, 0, 0), (255, 85, 0), (255, 170, 0), (255, 255, 0), (170, 255, 0), (85, 255, 0), (0, 255, 0), (0, 255, 85), (0, 255, 170), (0, 255, 255),
       (0, 170, 255), (0, 85, 255), (0, 0, 255), (85, 0, 255), (170, 0, 255), (255, 0, 255), (255, 0, 170), (255, 0, 85), (127, 127, 127)]
K = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
# layout -> (chroma shift x, chroma shift y, depth, left shift of a stored sample)
LAYOUT = {"nv12": (1, 1, 8, 0), "i420": (1, 1, 8, 0), "p010": (1, 1, 10, 6), "i010": (1, 1, 10, 0), "nv16": (1, 0, 8, 0), "i422": (1, 0, 8, 0),
          "yuy2": (1, 0, 8, 0), "uyvy": (1, 0, 8, 0), "i444": (0, 0, 8, 0)}
FORMATS = list(LAYOUT)
f32 = np.float32


def make_humans(parts_per_human):
    """HUMAN_DTYPE array from [{part index: (x, y)}, ...]"""
    hs = np.zeros(len(parts_per_human), HUMAN_DTYPE)
    for h, parts in zip(hs, parts_per_human):
        for k, (x, y) in parts.items():
            h["parts"][k] = (1, x, y, 1.0)
        h["score"] = 1.0
    return hs


def seeded_humans(seed, n, extent=0.25, keep=0.8, lo=-0.1, hi=1.1):
    """n compact humans (every part within `extent` of a centre drawn from [lo, hi]), each part present with probability `keep`"""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        cx, cy = r.uniform(lo, hi, 2)
        out.append({k: (float(f32(cx + r.uniform(-extent, extent))), float(f32(cy + r.uniform(-extent, extent)))) for k in range(18) if r.random() < keep})
    return make_humans(out)


def primitives(humans, W, H, thickness=0):
    """[(kind, x0, y0, x1, y1, t, colour, human)] by the rules of DESIGN.md 1.1, every float operation in float32"""
    out = []
    with np.errstate(all="ignore"):
        for hi, hm in enumerate(humans):
            parts = hm["parts"]
            present = [bool(p["has_value"]) and bool(np.isfinite(p["x"])) and bool(np.isfinite(p["y"])) for p in parts]
            if thickness > 0:
                t = int(thickness)
            else:
                n, s, w, e = f32(1), f32(0), f32(1), f32(0)
                for p, ok in zip(parts, present):
                    if ok:
                        n, s, w, e = min(n, f32(p["y"])), max(s, f32(p["y"])), min(w, f32(p["x"])), max(e, f32(p["x"]))
                root = np.sqrt(f32(f32(f32(e - w) * f32(s - n)) * f32(W * H)))
                if not root < f32(524288):
                    root = f32(524288)
                t = max(1, int(root) // 32)
            pix = {}
            for k, (p, ok) in enumerate(zip(parts, present)):
                if not ok:
                    continue
                fx, fy = f32(p["x"]) * f32(W), f32(p["y"]) * f32(H)
                if -8193 < fx < 16384 and -8193 < fy < 16384:
                    pix[k] = (int(fx), int(fy))  # int() truncates towards zero, as the C cast does
            for pid, (a, b) in enumerate(PAIRS):
                if a in pix and b in pix:
                    out.append((0, *pix[a], *pix[b], t, pid, hi))
            for k in range(18):
                if k in pix:
                    out.append((1, *pix[k], *pix[k], t, k, hi))
    return out


def covers(kind, x0, y0, x1, y1, t, x, y):
    px, py = x - x0, y - y0
    if kind == 1:
        return px * px + py * py <= t * t
    dx, dy = x1 - x0, y1 - y0
    L, s = dx * dx + dy * dy, px * dx + py * dy
    if L == 0 or s <= 0:
        return 4 * (px * px + py * py) <= t * t
    if s >= L:
        return 4 * ((px - dx) ** 2 + (py - dy) ** 2) <= t * t
    return 4 * (px * dy - py * dx) ** 2 <= t * t * L


def last_map(prims, W, H):
    """int32 [H, W]: index of the last primitive that covers each pixel, -1 where none does (Python integers throughout)"""
    last = np.full((H, W), -1, np.int32)
    for k, (kind, x0, y0, x1, y1, t, _, _) in enumerate(prims):
        for y in range(max(0, min(y0, y1) - t), min(H - 1, max(y0, y1) + t) + 1):
            for x in range(max(0, min(x0, x1) - t), min(W - 1, max(x0, x1) + t) + 1):
                if covers(kind, x0, y0, x1, y1, t, x, y):
                    last[y, x] = k
    return last


_cache = {}


def coverage(humans, W, H, thickness=0):
    """(primitives, last_map), computed once per distinct case and never modified"""
    key = (np.asarray(humans).tobytes(), W, H, thickness)
    if key not in _cache:
        prims = primitives(humans, W, H, thickness)
        last = last_map(prims, W, H)
        last.setflags(write=False)
        _cache[key] = (prims, last)
    return _cache[key]


@functools.lru_cache(None)
def colours(matrix, rng, depth):
    """the 19 colours as depth-bit (Y, U, V), float64 formulas"""
    kr, kb = K[matrix]
    kg = 1.0 - kr - kb
    top, up, half = float((1 << depth) - 1), float(1 << (depth - 8)), float(1 << (depth - 1))
    out = []
    for r, g, b in RGB:
        r, g, b = r / 255.0, g / 255.0, b / 255.0
        y = kr * r + kg * g + kb * b
        cb, cr = (b - y) / (2.0 * (1.0 - kb)), (r - y) / (2.0 * (1.0 - kr))
        if rng == "limited":
            v = [(16.0 + 219.0 * y) * up, (128.0 + 224.0 * cb) * up, (128.0 + 224.0 * cr) * up]
        else:
            v = [y * top, half + cb * top, half + cr * top]
        out.append([int(min(top, max(0.0, np.rint(c)))) for c in v])
    return np.array(out, np.int64)


def weight(opacity):
    return int(np.rint(np.float64(np.float32(opacity)) * 256.0))


def _put(view, mask, c, w, depth, shift):
    """view[mask] <- blend of c (an int64 array shaped like view) over the old samples"""
    old = (view[mask].astype(np.int64) >> shift) & ((1 << depth) - 1)
    new = c[mask] if w == 256 else (c[mask] * w + old * (256 - w) + 128) >> 8
    view[mask] = (new << shift).astype(view.dtype)


def sample_views(planes, fmt):
    """(Y, U, V) as numpy views into the planes: the layouts, restated"""
    if fmt in ("yuy2", "uyvy"):
        p = planes[0]
        return (p[:, 0::2], p[:, 1::4], p[:, 3::4]) if fmt == "yuy2" else (p[:, 1::2], p[:, 0::4], p[:, 2::4])
    if fmt in ("nv12", "nv16", "p010"):
        return planes[0], planes[1][:, 0::2], planes[1][:, 1::2]
    return planes[0], planes[1], planes[2]


def paint(frame, humans, fmt=None, matrix="bt601", rng="limited", opacity=1.0, thickness=0):
    """Paint in place: `frame` is uint8 [h, w, 3] BGR (fmt None) or the list of 2-D plane arrays of layout `fmt`."""
    w8 = weight(opacity)
    if fmt is None:
        H, W = frame.shape[:2]
        prims, last = coverage(humans, W, H, thickness)
        if not prims:
            return
        col = np.array([p[6] for p in prims])
        bgr = np.array(RGB, np.int64)[:, ::-1]
        for c in range(3):
            _put(frame[:, :, c], last >= 0, bgr[col[np.maximum(last, 0)], c], w8, 8, 0)
        return
    sx, sy, depth, shift = LAYOUT[fmt]
    Y, U, V = sample_views(frame, fmt)
    H, W = Y.shape
    prims, last = coverage(humans, W, H, thickness)
    if not prims:
        return
    col = np.array([p[6] for p in prims])
    table = colours(matrix, rng, depth)
    _put(Y, last >= 0, table[col[np.maximum(last, 0)], 0], w8, depth, shift)
    best = last.reshape(H >> sy, 1 << sy, W >> sx, 1 << sx).max(axis=(1, 3))  # the highest list index over a chroma sample's pixels
    _put(U, best >= 0, table[col[np.maximum(best, 0)], 1], w8, depth, shift)
    _put(V, best >= 0, table[col[np.maximum(best, 0)], 2], w8, depth, shift)


def random_frame(seed, fmt, W, H, pad=0):
    """(planes as views whose rows are `pad` bytes longer than the picture, the padded backing arrays); fmt None: ([h, w, 3] view, [backing])"""
    from hyperpose_amd import frontend
    r = np.random.default_rng(seed)
    if fmt is None:
        back = np.full((H, W * 3 + pad), 0xA5, np.uint8)
        view = back[:, :W * 3].reshape(H, W, 3)
        view[...] = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
        return view, [back]
    _, _, depth, shift = LAYOUT[fmt]
    views, backs = [], []
    for rows, cols in frontend.yuv_plane_shapes(fmt, W, H):
        if depth == 10:
            back = np.full((rows, cols + (pad + 1) // 2), 0xA5A5, np.uint16)
            back[:, :cols] = r.integers(0, 1024, (rows, cols), dtype=np.uint16) << shift
        else:
            back = np.full((rows, cols + pad), 0xA5, np.uint8)
            back[:, :cols] = r.integers(0, 256, (rows, cols), dtype=np.uint8)
        views.append(back[:, :cols])
        backs.append(back)
    return views, backs
