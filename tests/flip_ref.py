"""What the flip-ensemble tests share: test maps with the awkward float32 values in them, random tables, and the merge restated in NumPy
(include/hp_hip.h, "flip ensemble": 0.5f * (a +- b[perm][..., ::-1]) in float32)."""
import numpy as np


def special_maps(rng, shape):
    """Random finite float32 values with negative zeros, zeros, denormals and large magnitudes mixed in."""
    a = rng.standard_normal(shape).astype(np.float32)
    flat = a.reshape(-1)
    pick = rng.integers(0, 8, flat.size)
    flat[pick == 0] = np.float32(-0.0)
    flat[pick == 1] = np.float32(0.0)
    den = (rng.integers(1, 1 << 23, flat.size).astype(np.uint32) | (rng.integers(0, 2, flat.size).astype(np.uint32) << 31)).view(np.float32)
    flat[pick == 2] = den[pick == 2]
    flat[pick == 3] *= np.float32(1e30)
    assert np.isfinite(a).all()
    return a


def tables(rng, C):
    return rng.permutation(C).astype(np.int32), rng.choice(np.array([-1, 1], np.int8), C)


def numpy_merge(maps, n, perm, sign):
    out = maps.copy()
    half = np.float32(0.5)
    for f in range(n):
        a, b = maps[f], maps[n + f][perm][..., ::-1]
        out[f] = np.where(sign[:, None, None] > 0, half * (a + b), half * (a - b))
    assert out.dtype == np.float32
    return out
