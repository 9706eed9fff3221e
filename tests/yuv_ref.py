"""YUV 4:2:0 -> BGR on the CPU, the reference the YUV tests compare the GPU path with (numpy only).

The arithmetic is OpenCV's ``cvtColor(COLOR_YUV2BGR_NV12 / COLOR_YUV2BGR_I420)``: 8-bit fixed-point BT.601 limited range, restated from
its constants.  Parity unpinned: OpenCV is not in the build image, so this statement has not been run against cv2 here; a maintainer who
has cv2 can pin it with ``cv2.cvtColor(yuv, cv2.COLOR_YUV2BGR_NV12)`` on ``corner_frame("nv12")``.  What IS checked here is that the
constants mean what they should (tests/test_yuv_convert.py: within 1 of a float64 BT.601 evaluation over the whole (Y, U, V) cube).

    shift 20;  CY 1220542, CUB 2116026, CUG -409993, CVG -852492, CVR 1673527
    u = U-128, v = V-128, y = max(0, Y-16)*CY
    B = sat8((y + (1<<19) + CUB*u) >> 20)
    G = sat8((y + (1<<19) + CVG*v + CUG*u) >> 20)
    R = sat8((y + (1<<19) + CVR*v) >> 20)

Chroma is replicated over its 2 x 2 luma pixels, no interpolation.  Every sum fits in int32 (largest magnitude about 5.6e8); the shift
is arithmetic (numpy's >> on signed integers is).
"""
import numpy as np

SHIFT = 20
CY, CUB, CUG, CVG, CVR = 1220542, 2116026, -409993, -852492, 1673527


def yuv_to_bgr(y, u, v) -> np.ndarray:
    """Element-wise integer conversion of broadcastable Y, U, V arrays (values 0..255) -> uint8 array [..., 3] in B, G, R order."""
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    u, v = u - 128, v - 128
    yy = np.maximum(0, y - 16) * np.int32(CY) + np.int32(1 << (SHIFT - 1))
    b = (yy + np.int32(CUB) * u) >> SHIFT
    g = (yy + np.int32(CVG) * v + np.int32(CUG) * u) >> SHIFT
    r = (yy + np.int32(CVR) * v) >> SHIFT
    return np.clip(np.stack(np.broadcast_arrays(b, g, r), axis=-1), 0, 255).astype(np.uint8)


def planes(frame: np.ndarray, fmt: str):
    """(Y [h, w], U [h/2, w/2], V [h/2, w/2]) views of one [h*3/2, w] frame."""
    frame = np.asarray(frame, np.uint8)
    assert frame.ndim == 2 and frame.shape[0] % 3 == 0 and frame.shape[1] % 2 == 0, frame.shape
    h, w = frame.shape[0] * 2 // 3, frame.shape[1]
    assert h % 2 == 0
    y, c = frame[:h], frame[h:]
    if fmt == "nv12":
        uv = c.reshape(h // 2, w // 2, 2)
        return y, uv[..., 0], uv[..., 1]
    assert fmt == "i420", fmt
    c = c.reshape(2, h // 2, w // 2)
    return y, c[0], c[1]


def to_bgr(frame: np.ndarray, fmt: str) -> np.ndarray:
    """One [h*3/2, w] uint8 4:2:0 frame ("nv12" or "i420") -> [h, w, 3] uint8 BGR."""
    y, u, v = planes(frame, fmt)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    return np.ascontiguousarray(yuv_to_bgr(y, up(u), up(v)))


def pack(y: np.ndarray, u: np.ndarray, v: np.ndarray, fmt: str) -> np.ndarray:
    """Planes -> one [h*3/2, w] frame (the inverse of ``planes``)."""
    h, w = y.shape
    if fmt == "nv12":
        c = np.stack([u, v], axis=-1).reshape(h // 2, w)
    else:
        c = np.concatenate([u.ravel(), v.ravel()]).reshape(h // 2, w)
    return np.ascontiguousarray(np.concatenate([y, c], axis=0).astype(np.uint8))


CORNER_VALUES = (0, 16, 128, 235, 255)


def corner_frame(fmt: str, w: int = 64, h: int = 48, seed: int = 0) -> np.ndarray:
    """A frame that tiles every (Y, U, V) in {0, 16, 128, 235, 255}^3, so that every saturation branch of the conversion is hit: the 25
    (U, V) pairs cycle over the chroma samples, and the four luma pixels of a chroma sample step through the five Y values as the
    sample index grows (every (Y, U, V) triple appears once w*h/4 >= 125 * a few)."""
    assert w % 2 == 0 and h % 2 == 0 and (w // 2) * (h // 2) >= 250
    k = np.arange((h // 2) * (w // 2)).reshape(h // 2, w // 2)
    vals = np.array(CORNER_VALUES, np.uint8)
    u, v = vals[k % 5], vals[(k // 5) % 5]
    y = np.empty((h, w), np.uint8)
    for dy in range(2):
        for dx in range(2):
            y[dy::2, dx::2] = vals[(k // 25 + 2 * dy + dx) % 5]
    return pack(y, u, v, fmt)
