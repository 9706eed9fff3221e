"""What a kernel writes OUTSIDE the region it owns (a plain module: the GPU test files import it, test_footprint_cpu.py tests it).

The engine zero-fills every activation buffer once (hp_engine::plan_activations) and relies on the halo (P pixels around every image), the
separator rows of fp32 buffers (rows H + 2P .. rows32() - 1) and the pad channels (C .. cs - 1) reading as zero for ever after; frames
n .. max_batch - 1 belong to nobody during a partial batch.  `Engine.debug_raw` shows a buffer as it lies in memory,
[max_batch, rows, W + 2P, cs]; the functions here say which of its elements are interior and hold everything else to zero.
"""
import numpy as np

from hyperpose_amd import _lib

RAW_LIMIT = 64 << 20   # engines whose activations exceed this skip the raw copies: the full-size configuration tests keep their run time


def make_geom(H, W, C, P, max_batch, f32):
    """The geometry hp_engine_debug_raw_tensor reports for such a tensor (engine.cpp: tensor_info::rows32, cs = round_up(C, 32))."""
    rows = H + 2 * P
    if f32 and P > 0:
        rows = (rows + 1) // 2 * 2
    return dict(H=H, W=W, C=C, cs=(C + 31) // 32 * 32, P=P, rows=rows, elem_bytes=4 if f32 else 2, max_batch=max_batch)


def raw_shape(g):
    return (g["max_batch"], g["rows"], g["W"] + 2 * g["P"], g["cs"])


def interior_mask(g):
    """True exactly where b < max_batch, P <= y < P + H, P <= x < P + W and c < C."""
    m = np.zeros(raw_shape(g), bool)
    m[:, g["P"]:g["P"] + g["H"], g["P"]:g["P"] + g["W"], :g["C"]] = True
    return m


def region_of(g, y, x, c):
    """The name of the outside region an element lies in (rows first: a corner of the halo counts as top / bottom)."""
    P, H, W = g["P"], g["H"], g["W"]
    if y < P:
        return "top halo"
    if y >= H + 2 * P:
        return "separator row"
    if y >= P + H:
        return "bottom halo"
    if x < P:
        return "left halo"
    if x >= P + W:
        return "right halo"
    if c >= g["C"]:
        return "pad channel"
    return "interior"


def check_zero_outside(arr, g, what="tensor", show=6):
    """Every element outside the interior compares equal to 0 (so -0.0 passes, NaN and inf do not)."""
    assert arr.shape == raw_shape(g) and arr.dtype.itemsize == g["elem_bytes"], (what, arr.shape, arr.dtype, g)
    bad = ~interior_mask(g) & ~(arr == 0)   # NaN == 0 is False: not-equal-to-zero covers every non-finite value too
    if not bad.any():
        return
    idx = np.argwhere(bad)
    lines = []
    for b, y, x, c in idx[:show]:
        lines.append(f"frame {b} (y={y}, x={x}, c={c}) = {float(arr[b, y, x, c])!r} [{region_of(g, y, x, c)}]")
    regions = sorted({region_of(g, y, x, c) for _, y, x, c in idx[:4096]})
    raise AssertionError(f"{what}: {len(idx)} element(s) outside the interior are not zero (H={g['H']} W={g['W']} C={g['C']} cs={g['cs']} P={g['P']} "
                         f"rows={g['rows']}); regions: {', '.join(regions)}; first: " + "; ".join(lines))


def check_frames_unchanged(before, first, after, n, what="tensor", show=6):
    """Frames n .. of the raw array `after` are bitwise those of `before`, which holds frames `first` .. max_batch - 1 (first <= n)."""
    assert 0 <= first <= n and before.shape[0] == after.shape[0] - first, (what, first, n, before.shape, after.shape)
    tail, now = before[n - first:], after[n:]
    assert tail.shape == now.shape and tail.dtype == now.dtype, (what, tail.shape, now.shape)
    a = np.ascontiguousarray(tail).view(np.uint8).reshape(tail.shape + (tail.dtype.itemsize,))
    b = np.ascontiguousarray(now).view(np.uint8).reshape(now.shape + (now.dtype.itemsize,))
    diff = (a != b).any(axis=-1)
    if not diff.any():
        return
    idx = np.argwhere(diff)
    lines = [f"frame {n + f} (y={y}, x={x}, c={c}): {float(tail[f, y, x, c])!r} -> {float(now[f, y, x, c])!r}" for f, y, x, c in idx[:show]]
    raise AssertionError(f"{what}: a batch of {n} changed {len(idx)} element(s) of frames {n}..{after.shape[0] - 1}; first: " + "; ".join(lines))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tensor_ids(layers):
    """Every tensor the layer list writes."""
    return sorted({int(L.out) for L in layers})


def materialised(eng, ids):
    """(tensor, raw array, geometry) of every tensor of `ids` that exists in memory (fused-away and output-only tensors are refused by the tap)."""
    for t in ids:
        try:
            arr, g = eng.debug_raw(t)
        except _lib.HpError as err:
            assert err.code == _lib.HP_ERR_STATE, (t, err)
            continue
        yield t, arr, g


def too_large(eng):
    return eng.device_bytes["activations"] > RAW_LIMIT


def assert_zero_outside(eng, ids, n=None, what=""):
    """Every materialised tensor of `ids` is zero outside its interior.  With `n` (the last batch) also the tap's own sanity: the interior
    of the raw array is debug_tensor's bit for bit wherever debug_tensor shows the tensor (it refuses tensors that share an arena buffer).
    Returns the number of tensors looked at; engines above RAW_LIMIT are not copied (0)."""
    if too_large(eng):
        print(f"footprint: raw copies skipped, the engine holds {eng.device_bytes['activations'] / 2 ** 20:.0f} MiB of activations")
        return 0
    seen = 0
    for t, arr, g in materialised(eng, ids):
        seen += 1
        check_zero_outside(arr, g, f"{what} tensor {t}".strip())
        if n is None:
            continue
        try:
            inner = eng.debug_tensor(t, n)
        except _lib.HpError as err:
            assert err.code == _lib.HP_ERR_STATE, (t, err)
            continue
        P = g["P"]
        mine = arr[:n, P:P + g["H"], P:P + g["W"], :g["C"]].transpose(0, 3, 1, 2)
        assert np.array_equal(_bits(mine), _bits(inner)), f"{what} tensor {t}: the raw buffer's interior is not what debug_tensor shows"
    return seen


def snapshot_frames(eng, ids, frames):
    """Raw copies of frames `frames` .. max_batch - 1 of every materialised tensor: (frames, {tensor: array})."""
    return frames, {t: arr[frames:].copy() for t, arr, _ in materialised(eng, ids)}


def assert_frames_unchanged(eng, snap, frames, what=""):
    """After a batch of `frames`: frames `frames` .. of every tensor are bitwise what `snap` = snapshot_frames(eng, ids, first <= frames) holds."""
    first, held = snap
    assert held
    for t, arr, _ in materialised(eng, list(held)):
        check_frames_unchanged(held[t], first, arr, frames, f"{what} tensor {t}".strip())
