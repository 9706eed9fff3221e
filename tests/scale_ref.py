"""What the scale-ensemble tests share: the bicubic tables and the merge restated in NumPy float32, in the order include/hp_hip.h ("scale
ensemble") states them, and the valid map region of a scale."""
import math

import numpy as np

F = np.float32


def cells(s, W):
    """mw = max(1, (int)floor((double)s * W + 0.5)) for a float32 scale s."""
    return max(1, int(math.floor(float(np.float32(s)) * W + 0.5)))


def tables(W, mw):
    """(idx int32 [W, 4], wgt float32 [W, 4]): OpenCV's bicubic, A = -0.75, every operation on float32 scalars."""
    A, one = F(-0.75), F(1)
    idx, wgt = np.zeros((W, 4), np.int32), np.zeros((W, 4), np.float32)
    for x in range(W):
        fx = F((x + 0.5) * (mw / W) - 0.5)  # double, then narrowed once
        sx = int(np.floor(fx))
        fx = F(fx - F(sx))
        u = F(fx + one)
        c0 = F(F(F(F(F(A * u) - F(F(5) * A)) * u) + F(F(8) * A)) * u) - F(F(4) * A)
        c1 = F(F(F(F(F(A + F(2)) * fx) - F(A + F(3))) * fx) * fx) + one
        v = F(one - fx)
        c2 = F(F(F(F(F(A + F(2)) * v) - F(A + F(3))) * v) * v) + one
        c3 = F(F(F(one - c0) - c1) - c2)
        wgt[x] = (c0, c1, c2, c3)
        idx[x] = [min(max(sx - 1 + j, 0), mw - 1) for j in range(4)]
    return idx, wgt


def merge(maps, n, scales):
    """maps [>= K n, C, H, W] float32, scale-major -> a copy with maps [0, n) merged."""
    K = len(scales) + 1
    out = maps.copy()
    _, C, H, W = maps.shape
    with np.errstate(over="ignore", invalid="ignore"):
        for f in range(n):
            acc = maps[f].copy()
            for k in range(1, K):
                ix, wx = tables(W, cells(scales[k - 1], W))
                iy, wy = tables(H, cells(scales[k - 1], H))
                p = maps[k * n + f]                                   # [C, H, W]
                rows = []
                for r in range(4):
                    pr = p[:, iy[:, r], :]                           # [C, H, W]: row r of every output row
                    t = wx[None, None, :, 0] * pr[:, :, ix[:, 0]]
                    for j in range(1, 4):
                        t = t + wx[None, None, :, j] * pr[:, :, ix[:, j]]
                    rows.append(t)
                v = wy[None, :, None, 0] * rows[0]
                for r in range(1, 4):
                    v = v + wy[None, :, None, r] * rows[r]
                acc = acc + v
            out[f] = acc * (F(1) / F(K))
    assert out.dtype == np.float32
    return out
