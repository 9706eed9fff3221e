"""The tests' own statement of the redaction picture (hp_redact_*, include/hp_hip.h; DESIGN.md 1.1 "Redaction"): a region builder and a numpy
painter that call the library for nothing they check.  Part points are numpy float32; regions, hits and means are Python integers (no width to
overflow); the samples are read and written through numpy views of the planes.  Shared by tests/test_redact_host.py, tests/test_redact_gpu.py,
tests/test_cli_redact.py and tools/redact_bench.py."""
import math

import numpy as np
from overlay_ref import LAYOUT, make_humans, random_frame, seeded_humans  # noqa: F401  (re-exported for the tests)

RECT, DISC = 0, 1
FACE = (0, 14, 15, 16, 17)
LO, HI, MAX_R = -8192, 16383, 16384
f32 = np.float32


def points(human, W, H):
    """{part index: (x, y)} of the present parts: has_value, finite, and the fp32 point inside [LO, HI] in both coordinates"""
    out = {}
    with np.errstate(all="ignore"):
        for k, p in enumerate(human["parts"]):
            if not p["has_value"] or not np.isfinite(p["x"]) or not np.isfinite(p["y"]):
                continue
            fx, fy = f32(p["x"]) * f32(W), f32(p["y"]) * f32(H)
            if LO - 1 < fx < HI + 1 and LO - 1 < fy < HI + 1:
                out[k] = (int(fx), int(fy))  # int() truncates towards zero, as the C cast does
    return out


def _box(pts):
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    return min(xs), min(ys), max(xs), max(ys)


def regions(humans, W, H, what="head", margin=1.0):
    """[(kind, x0, y0, x1, y1, human)] by the rules of DESIGN.md 1.1"""
    m = int(np.rint(np.float64(np.float32(margin)) * 256.0))
    clamp = lambda v: min(HI, max(LO, v))  # noqa: E731
    out = []
    for i, hm in enumerate(humans):
        pix = points(hm, W, H)
        if what == "body" and pix:
            lx, ly, hx, hy = _box(list(pix.values()))
            p = max(1, (max(hx - lx, hy - ly) * m + 1024) >> 11)
            out.append((RECT, clamp(lx - p), clamp(ly - p), clamp(hx + p), clamp(hy + p), i))
        face = [pix[k] for k in FACE if k in pix]
        if not face:
            continue
        lx, ly, hx, hy = _box(face)
        dist = lambda a, b: math.isqrt((pix[a][0] - pix[b][0]) ** 2 + (pix[a][1] - pix[b][1]) ** 2)  # noqa: E731
        nk = dist(1, 0) if 1 in pix and 0 in pix else 0
        sh = dist(2, 5) >> 1 if 2 in pix and 5 in pix else 0
        b = max(hx - lx, hy - ly, nk, sh, 1)
        out.append((DISC, (lx + hx) // 2, (ly + hy) // 2, min(MAX_R, max(1, (b * m + 128) >> 8)), 0, i))
    return out


def hit(region, X0, Y0, X1, Y1):
    kind, x0, y0, x1, y1 = region[:5]
    if kind == RECT:
        return x0 <= X1 and x1 >= X0 and y0 <= Y1 and y1 >= Y0
    dx, dy = x0 - min(max(x0, X0), X1), y0 - min(max(y0, Y0), Y1)
    return dx * dx + dy * dy <= x1 * x1


def hit_cells(regs, W, H, cell):
    """[(X0, Y0, X1, Y1)] of the cells (clipped to the frame) that any region reaches"""
    out = []
    for Y0 in range(0, H, cell):
        for X0 in range(0, W, cell):
            X1, Y1 = min(W, X0 + cell) - 1, min(H, Y0 + cell) - 1
            if any(hit(r, X0, Y0, X1, Y1) for r in regs):
                out.append((X0, Y0, X1, Y1))
    return out


def sample_views(planes, fmt):
    """(Y, U, V) as numpy views into the planes: YUY2 is Y0 U Y1 V, UYVY is U Y0 V Y1, semi-planar pairs are (U, V)"""
    if fmt == "yuy2":
        return planes[0][:, 0::2], planes[0][:, 1::4], planes[0][:, 3::4]
    if fmt == "uyvy":
        return planes[0][:, 1::2], planes[0][:, 0::4], planes[0][:, 2::4]
    if len(planes) == 2:
        return planes[0], planes[1][:, 0::2], planes[1][:, 1::2]
    return planes[0], planes[1], planes[2]


def _fill(view, depth, shift, value):
    """view <- value when given, else the rounded mean of its code values"""
    if value is None:
        total, cnt = int(((view.astype(np.int64) >> shift) & ((1 << depth) - 1)).sum()), view.size
        value = (total + cnt // 2) // cnt
    view[...] = value << shift


def paint(frame, regs, fmt=None, rng="limited", effect="pixelate", cell=16):
    """Redact in place: `frame` is uint8 [h, w, 3] BGR (fmt None) or the list of 2-D plane arrays of layout `fmt`.  Returns the hit cells."""
    black = effect == "black"
    if fmt is None:
        H, W = frame.shape[:2]
        cells = hit_cells(regs, W, H, cell)
        for X0, Y0, X1, Y1 in cells:
            for c in range(3):
                _fill(frame[Y0:Y1 + 1, X0:X1 + 1, c], 8, 0, 0 if black else None)
        return cells
    sx, sy, depth, shift = LAYOUT[fmt]
    Y, U, V = sample_views(frame, fmt)
    H, W = Y.shape
    cells = hit_cells(regs, W, H, cell)
    y_black, c_black = ((16 << (depth - 8)) if rng == "limited" else 0), 1 << (depth - 1)
    for X0, Y0, X1, Y1 in cells:
        _fill(Y[Y0:Y1 + 1, X0:X1 + 1], depth, shift, y_black if black else None)
        for plane in (U, V):
            _fill(plane[Y0 >> sy:(Y1 >> sy) + 1, X0 >> sx:(X1 >> sx) + 1], depth, shift, c_black if black else None)
    return cells


def as_records(regs):
    from hyperpose_amd._lib import REDACT_REGION_DTYPE
    return np.array([tuple(r) for r in regs], REDACT_REGION_DTYPE) if len(regs) else np.zeros(0, REDACT_REGION_DTYPE)
