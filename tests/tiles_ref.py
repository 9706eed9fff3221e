"""numpy restatement of the host side of tiled inference, from the rules in include/hp_hip.h ("regions and tiles"): the tile planner, the
way back from a region to the frame and the merge.  Integers and IEEE doubles in the stated order, so results compare byte for byte."""
import numpy as np

from hyperpose_amd._lib import HUMAN_DTYPE

N_PARTS = 18


def _axis(W, c, overlap, a):
    o = (overlap + a - 1) // a * a
    tw = min(W, ((W + (c - 1) * o + c - 1) // c + a - 1) // a * a)
    xs = [0 if c == 1 else (W - tw if i == c - 1 else (i * (W - tw) // (c - 1)) // a * a) for i in range(c)]
    return tw, xs


def plan(W, H, cols, rows, overlap=(0, 0), with_full=False, align=(1, 1)):
    tw, xs = _axis(W, cols, overlap[0], align[0])
    th, ys = _axis(H, rows, overlap[1], align[1])
    out = [(0, 0, W, H)] if with_full else []
    return out + [(x, y, tw, th) for y in ys for x in xs]


def to_frame(humans, roi, fw, fh):
    hs = np.array(humans, HUMAN_DTYPE).reshape(-1).copy()
    x, y, w, h = roi
    p = hs["parts"]
    on = p["has_value"] != 0
    nx = ((np.float64(x) + p["x"].astype(np.float64) * np.float64(w)) / np.float64(fw)).astype(np.float32)
    ny = ((np.float64(y) + p["y"].astype(np.float64) * np.float64(h)) / np.float64(fh)).astype(np.float32)
    p["x"] = np.where(on, nx, p["x"])
    p["y"] = np.where(on, ny, p["y"])
    return hs


def _extent(h, fw, fh):
    on = [j for j in range(N_PARTS) if h["parts"][j]["has_value"]]
    if not on:
        return np.float64(0)
    px = [np.float64(h["parts"][j]["x"]) * np.float64(fw) for j in on]
    py = [np.float64(h["parts"][j]["y"]) * np.float64(fh) for j in on]
    return max(max(px) - min(px), max(py) - min(py))


def merge(humans, region_of, fw, fh, min_common, tol):
    hs = np.array(humans, HUMAN_DTYPE).reshape(-1)
    order = sorted(range(len(hs)), key=lambda i: (-float(hs[i]["score"]), int(region_of[i]), i))
    kept, regions = [], []
    fw64, fh64 = np.float64(fw), np.float64(fh)
    for i in order:
        c = hs[i].copy()
        sc = _extent(c, fw, fh)
        into = None
        for k, kh in enumerate(kept):
            if int(region_of[i]) in regions[k]:
                continue
            m, total = 0, np.float64(0)
            for j in range(N_PARTS):
                a, b = kh["parts"][j], c["parts"][j]
                if not a["has_value"] or not b["has_value"]:
                    continue
                dx = np.float64(a["x"]) * fw64 - np.float64(b["x"]) * fw64
                dy = np.float64(a["y"]) * fh64 - np.float64(b["y"]) * fh64
                total = total + np.sqrt(dx * dx + dy * dy)
                m += 1
            if m < min_common:
                continue
            if total <= (np.float64(tol) * np.float64(m)) * max(_extent(kh, fw, fh), sc):
                into = k
                break
        if into is None:
            kept.append(c)
            regions.append({int(region_of[i])})
            continue
        for j in range(N_PARTS):
            a, b = kept[into]["parts"][j], c["parts"][j]
            if b["has_value"] and (not a["has_value"] or b["score"] > a["score"]):
                kept[into]["parts"][j] = b
        regions[into].add(int(region_of[i]))
    return np.array(kept, HUMAN_DTYPE) if kept else np.zeros(0, HUMAN_DTYPE)
