"""The HP_ORIENT_* definition of include/hp_hip.h restated in numpy: code = q + 4 * m, q quarter turns clockwise that bring the stored picture
upright, m = mirrored left-right first.  The reference of every orientation test; nothing here calls the library."""
import numpy as np

CODES = list(range(8))
EXIF = {1: 0, 2: 4, 3: 2, 4: 6, 5: 7, 6: 1, 7: 5, 8: 3}


def orient(S: np.ndarray, code: int) -> np.ndarray:
    """The upright frame of a stored [h, w, ...] array."""
    q, m = code & 3, code >> 2
    return np.ascontiguousarray(np.rot90(S[:, ::-1] if m else S, k=-q))


def oriented_size(code: int, sw: int, sh: int):
    return (sh, sw) if code & 1 else (sw, sh)


def stored_xy(code: int, sw: int, sh: int, ux: int, uy: int):
    """The header's pixel map, one pixel at a time: upright (ux, uy) -> stored (x, y)."""
    q, m = code & 3, code >> 2
    x, y = [(ux, uy), (uy, sh - 1 - ux), (sw - 1 - ux, sh - 1 - uy), (sw - 1 - uy, ux)][q]
    return (sw - 1 - x if m else x), y


def orient_by_map(S: np.ndarray, code: int) -> np.ndarray:
    sh, sw = S.shape[:2]
    uw, uh = oriented_size(code, sw, sh)
    U = np.empty((uh, uw) + S.shape[2:], S.dtype)
    for uy in range(uh):
        for ux in range(uw):
            x, y = stored_xy(code, sw, sh, ux, uy)
            U[uy, ux] = S[y, x]
    return U


def orient_roi(roi, code: int, sw: int, sh: int):
    """The stored rectangle of an upright region: the bounding box of its two opposite corners' stored pixels."""
    x, y, w, h = roi
    (x0, y0), (x1, y1) = stored_xy(code, sw, sh, x, y), stored_xy(code, sw, sh, x + w - 1, y + h - 1)
    return min(x0, x1), min(y0, y1), abs(x1 - x0) + 1, abs(y1 - y0) + 1


def humans_orient(humans: np.ndarray, code: int, to_stored: bool) -> np.ndarray:
    """hp_humans_orient in fp32, exactly as the header writes it; parts without has_value and all scores stay."""
    out = humans.copy()
    q, m = code & 3, code >> 2
    one = np.float32(1.0)
    p = out["parts"]
    a, b = p["x"].astype(np.float32), p["y"].astype(np.float32)
    if to_stored:
        x, y = [(a, b), (b, one - a), (one - a, one - b), (one - b, a)][q]
        x = one - x if m else x
    else:
        a = one - a if m else a
        x, y = [(a, b), (one - b, a), (one - a, one - b), (b, one - a)][q]
    has = p["has_value"] != 0
    p["x"] = np.where(has, x, p["x"])
    p["y"] = np.where(has, y, p["y"])
    return out
