"""CPU: the host side of tiled inference (hp_tile_plan, hp_humans_to_frame, hp_humans_merge) against its numpy restatement
(tests/tiles_ref.py) and against the properties include/hp_hip.h promises.  No device is touched."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tiles_ref
from hyperpose_amd import _lib, frontend
from hyperpose_amd._lib import HUMAN_DTYPE, HpError

FRAMES = [(64, 48), (97, 61), (1920, 1080), (3840, 2160)]
GRIDS = [(c, r) for c in range(1, 5) for r in range(1, 4)]
OVERLAPS = [0, 1, 32, 5000]  # the last is larger than any tile
ALIGNS = [(1, 1), (2, 1), (2, 2)]


# ---- planner ------------------------------------------------------------------------------------------------------------------------

def _axis_ok(starts, size, W, overlap, a):
    assert all(s % a == 0 and 0 <= s and s + size <= W for s in starts) and size % a == 0 and size > 0
    assert starts[0] == 0 and starts[-1] + size == W and list(starts) == sorted(starts)
    for s0, s1 in zip(starts, starts[1:]):
        assert s1 <= s0 + size, "a gap between neighbours"  # with the two ends pinned: every pixel is covered
        if size < W:
            assert s0 + size - s1 >= overlap, (starts, size, overlap)


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("align", ALIGNS)
def test_plan_matches_restatement_and_covers(W, H, align):
    if W % align[0] or H % align[1]:
        for with_full in (False, True):
            with pytest.raises(HpError) as e:
                frontend.plan_tiles(W, H, 2, 2, (0, 0), with_full, align=align)
            assert e.value.code == _lib.HP_ERR_INVALID
        return
    for (cols, rows), ox, oy, with_full in itertools.product(GRIDS, OVERLAPS, OVERLAPS[:3], (False, True)):
        got = frontend.plan_tiles(W, H, cols, rows, (ox, oy), with_full, align=align)
        assert got == tiles_ref.plan(W, H, cols, rows, (ox, oy), with_full, align), (cols, rows, ox, oy, with_full)
        assert len(got) == cols * rows + int(with_full)
        if with_full:
            assert got[0] == (0, 0, W, H)
        tiles = got[int(with_full):]
        tw, th = tiles[0][2], tiles[0][3]
        assert all(t[2] == tw and t[3] == th for t in tiles)
        xs, ys = [t[0] for t in tiles[:cols]], [t[1] for t in tiles[::cols]]
        assert tiles == [(x, y, tw, th) for y in ys for x in xs], "row-major order"
        _axis_ok(xs, tw, W, ox, align[0])
        _axis_ok(ys, th, H, oy, align[1])


def test_plan_union_covers_every_pixel():
    for W, H, align in [(64, 48, (2, 2)), (97, 61, (1, 1))]:
        for (cols, rows), o in itertools.product(GRIDS, (0, 1, 32)):
            seen = np.zeros((H, W), bool)
            for x, y, w, h in frontend.plan_tiles(W, H, cols, rows, (o, o), align=align):
                seen[y:y + h, x:x + w] = True
            assert seen.all()


def test_plan_rejections():
    for kw, code in [(dict(cols=8, rows=8, with_full=True), _lib.HP_ERR_INVALID), (dict(cols=65, rows=1), _lib.HP_ERR_INVALID),
                     (dict(cols=0, rows=2), _lib.HP_ERR_INVALID), (dict(cols=2, rows=2, overlap=(-1, 0)), _lib.HP_ERR_INVALID),
                     (dict(cols=2, rows=2, cap=3), _lib.HP_ERR_CAPACITY), (dict(cols=2, rows=2, with_full=True, cap=4), _lib.HP_ERR_CAPACITY)]:
        with pytest.raises(HpError) as e:
            frontend.plan_tiles(640, 360, **kw)
        assert e.value.code == code, kw
    assert len(frontend.plan_tiles(640, 360, 8, 8)) == 64
    assert len(frontend.plan_tiles(640, 360, 9, 7, with_full=True)) == 64
    for fmt, want in [("nv12", (2, 2)), ("i420", (2, 2)), ("p010", (2, 2)), ("i010", (2, 2)), ("nv16", (2, 1)), ("i422", (2, 1)), ("yuy2", (2, 1)),
                      ("uyvy", (2, 1)), ("i444", (1, 1))]:
        assert frontend.yuv_roi_alignment(fmt) == want


# ---- map-back -----------------------------------------------------------------------------------------------------------------------

def _random_humans(rng, n, lo=-0.5, hi=1.5):
    hs = np.zeros(n, HUMAN_DTYPE)
    hs["parts"]["has_value"] = rng.integers(0, 2, (n, 18))
    hs["parts"]["x"] = rng.uniform(lo, hi, (n, 18)).astype(np.float32)
    hs["parts"]["y"] = rng.uniform(lo, hi, (n, 18)).astype(np.float32)
    hs["parts"]["score"] = rng.uniform(0, 1, (n, 18)).astype(np.float32)
    hs["score"] = rng.uniform(0, 30, n).astype(np.float32)
    return hs


def test_to_frame_is_identity_on_the_whole_frame():
    rng = np.random.default_rng(5)
    hs = _random_humans(rng, 278)  # 2 x 278 x 18 = 10 008 coordinates
    hs["parts"]["has_value"] = 1
    # every magnitude, not only coordinates inside the frame
    hs["parts"]["x"] = (rng.uniform(-1, 1, (278, 18)) * 10.0 ** rng.integers(-30, 5, (278, 18))).astype(np.float32)
    for w, h in FRAMES + [(8192, 8192)]:
        assert frontend.humans_to_frame(hs, (0, 0, w, h), w, h).tobytes() == hs.tobytes(), (w, h)


def test_to_frame_matches_restatement():
    rng = np.random.default_rng(6)
    for w, h in FRAMES:
        for _ in range(8):
            rw, rh = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            roi = (int(rng.integers(0, w - rw + 1)), int(rng.integers(0, h - rh + 1)), rw, rh)
            hs = _random_humans(rng, 40)
            got = frontend.humans_to_frame(hs, roi, w, h)
            assert got.tobytes() == tiles_ref.to_frame(hs, roi, w, h).tobytes(), roi
            off = hs["parts"]["has_value"] == 0
            assert np.array_equal(got["parts"]["x"][off], hs["parts"]["x"][off]), "absent parts are left alone"
    hs = np.zeros(1, HUMAN_DTYPE)
    hs["parts"]["has_value"], hs["parts"]["x"], hs["parts"]["y"] = 1, 0.5, 0.25
    got = frontend.humans_to_frame(hs, (100, 50, 200, 100), 400, 200)
    assert np.all(got["parts"]["x"] == np.float32(0.5)) and np.all(got["parts"]["y"] == np.float32(0.375))


# ---- merge --------------------------------------------------------------------------------------------------------------------------

FW, FH = 640, 360


def _human(parts, score):
    """parts: {index: (x px, y px, part score)}"""
    h = np.zeros((), HUMAN_DTYPE)
    for j, (x, y, s) in parts.items():
        h["parts"][j] = (1, np.float32(x / FW), np.float32(y / FH), np.float32(s))
    h["score"] = np.float32(score)
    return h


def _both(humans, regions, min_common, tol, cap=None):
    hs = np.array(humans, HUMAN_DTYPE).reshape(-1)
    got = frontend.merge_humans(hs, regions, FW, FH, min_common, tol, cap)
    ref = tiles_ref.merge(hs, regions, FW, FH, min_common, tol)
    assert got.tobytes() == ref.tobytes()
    return got


def _crowd(seed):
    """1-12 ground-truth people cut by a 2 x 2 plan with overlap: every tile sees the parts that lie inside it, with its own jitter"""
    rng = np.random.default_rng(seed)
    tiles = frontend.plan_tiles(FW, FH, 2, 2, (64, 64))
    humans, regions = [], []
    for _ in range(int(rng.integers(1, 13))):
        cx, cy = rng.uniform(40, FW - 40), rng.uniform(40, FH - 40)
        size = rng.uniform(30, 160)
        pts = np.stack([cx + rng.uniform(-0.3, 0.3, 18) * size, cy + rng.uniform(-0.5, 0.5, 18) * size], 1)
        pts = np.clip(pts, 0, [FW - 1, FH - 1])
        for r, (x, y, w, h) in enumerate(tiles):
            seen = {j: (pts[j, 0] + rng.normal(0, 1.0), pts[j, 1] + rng.normal(0, 1.0), rng.uniform(0.1, 1))
                    for j in range(18) if x <= pts[j, 0] < x + w and y <= pts[j, 1] < y + h and rng.random() < 0.9}
            if len(seen) >= 2:
                humans.append(_human(seen, rng.choice([rng.uniform(1, 20), 7.0])))  # some equal human scores
                regions.append(r)
    return humans, regions


@pytest.mark.parametrize("seed", range(12))
def test_merge_matches_restatement_on_crowds(seed):
    humans, regions = _crowd(seed)
    for min_common, tol in [(1, 0.5), (3, 0.08), (2, 0.03), (6, 0.0), (3, 10.0)]:
        got = _both(humans, regions, min_common, tol)
        assert 1 <= len(got) <= len(humans)
    assert len(_both(humans, regions, 19, 10.0)) == len(humans), "no two humans share 19 parts"


def test_merge_split_person_becomes_one():
    body = {j: (300 + 4 * j, 100 + 9 * j, 0.5) for j in range(12)}
    left = _human({j: body[j] for j in range(0, 8)}, 9.0)
    right = _human({j: (body[j][0] + 1, body[j][1] - 1, 0.6 if j < 6 else 0.4) for j in range(4, 12)}, 8.0)
    got = _both([left, right], [0, 1], 4, 0.05)
    assert len(got) == 1 and got[0]["score"] == np.float32(9.0) and int(got[0]["parts"]["has_value"].sum()) == 12
    p = got[0]["parts"]
    assert p[3].tobytes() == left["parts"][3].tobytes() and p[10].tobytes() == right["parts"][10].tobytes()
    assert p[4].tobytes() == right["parts"][4].tobytes() and p[5].tobytes() == right["parts"][5].tobytes(), "the higher part score wins"
    assert p[6].tobytes() == left["parts"][6].tobytes() and p[7].tobytes() == left["parts"][7].tobytes()
    # one common part short of min_common: two humans, untouched, by score
    got = _both([right, left], [1, 0], 5, 0.05)
    assert len(got) == 2 and got[0].tobytes() == left.tobytes() and got[1].tobytes() == right.tobytes()
    # enough common parts but further apart than tol allows
    far = _human({j: (body[j][0] + 40, body[j][1], 0.6) for j in range(4, 12)}, 8.0)
    assert len(_both([left, far], [0, 1], 4, 0.05)) == 2
    assert len(_both([left, far], [0, 1], 4, 1.0)) == 1


def test_merge_never_fuses_two_humans_of_one_region():
    a = _human({j: (100 + 5 * j, 100 + 5 * j, 0.5) for j in range(10)}, 5.0)
    b = _human({j: (101 + 5 * j, 100 + 5 * j, 0.5) for j in range(10)}, 4.0)
    assert len(_both([a, b], [2, 2], 3, 0.5)) == 2
    assert len(_both([a, b], [2, 3], 3, 0.5)) == 1
    # a third detection from the same region as b: it fuses into a only while a holds nothing of that region
    c = _human({j: (100 + 5 * j, 101 + 5 * j, 0.5) for j in range(10)}, 3.0)
    got = _both([a, b, c], [2, 3, 3], 3, 0.5)
    assert len(got) == 2 and got[1].tobytes() == c.tobytes()


def test_merge_order_on_equal_scores_and_ties():
    parts = {j: (200 + 6 * j, 150 + 3 * j, 0.5) for j in range(8)}
    a, b, c = _human(parts, 5.0), _human({j: (x + 1, y, s) for j, (x, y, s) in parts.items()}, 5.0), _human({j: (x + 2, y, s) for j, (x, y, s) in parts.items()}, 5.0)
    # nothing fuses (tol 0): the order is by region, then by input index
    got = _both([a, b, c], [3, 1, 1], 3, 0.0)
    assert [h.tobytes() for h in got] == [b.tobytes(), c.tobytes(), a.tobytes()]
    # everything fuses: the kept human is the first in that order, and on equal part scores its parts stay
    got = _both([a, b], [3, 1], 3, 0.5)
    assert len(got) == 1 and got[0].tobytes() == b.tobytes()


def test_merge_three_way_only_after_the_first_fusion():
    body = {j: (320 + 5 * j, 60 + 12 * j, 0.5) for j in range(9)}
    k = _human({j: body[j] for j in (0, 1, 2)}, 9.0)
    c1 = _human({j: body[j] for j in range(6)}, 8.0)
    c2 = _human({j: body[j] for j in (3, 4, 5, 6, 7, 8)}, 7.0)
    got = _both([k, c1, c2], [0, 1, 2], 3, 0.05)
    assert len(got) == 1 and int(got[0]["parts"]["has_value"].sum()) == 9 and got[0]["score"] == np.float32(9.0)
    # without c1 the third has nothing in common with k
    assert len(_both([k, c2], [0, 2], 3, 0.05)) == 2
    # taken before c1 (a higher score), c2 finds no partner yet and stays a human of its own; c1 then fuses into k, the first kept
    c2_first = c2.copy()
    c2_first["score"] = np.float32(8.5)
    got = _both([k, c1, c2_first], [0, 1, 2], 3, 0.05)
    assert len(got) == 2 and int(got[0]["parts"]["has_value"].sum()) == 6 and got[1].tobytes() == c2_first.tobytes()


def test_merge_capacity_and_arguments():
    humans = [_human({j: (50 + 60 * i, 40 + 5 * j, 0.5) for j in range(6)}, 10.0 - i) for i in range(5)]
    assert len(_both(humans, [0] * 5, 3, 0.05, cap=5)) == 5
    with pytest.raises(HpError) as e:
        frontend.merge_humans(np.array(humans, HUMAN_DTYPE), [0] * 5, FW, FH, 3, 0.05, cap=4)
    assert e.value.code == _lib.HP_ERR_CAPACITY
    for kw in [dict(region_of=[0, 0, 0, 0, 64]), dict(region_of=[0, 0, -1, 0, 0]), dict(min_common=0), dict(tol=-0.1), dict(tol=float("nan"))]:
        args = dict(region_of=[0] * 5, min_common=3, tol=0.05)
        args.update(kw)
        with pytest.raises(HpError) as e:
            frontend.merge_humans(np.array(humans, HUMAN_DTYPE), args["region_of"], FW, FH, args["min_common"], args["tol"])
        assert e.value.code == _lib.HP_ERR_INVALID, kw
    assert len(frontend.merge_humans(np.zeros(0, HUMAN_DTYPE), [], FW, FH)) == 0
    out = np.zeros(4, HUMAN_DTYPE)  # on overflow the first cap humans are written
    hs = np.array(humans, HUMAN_DTYPE)
    reg = np.zeros(5, np.int32)
    rc = _lib.lib().hp_humans_merge(hs.ctypes.data_as(C.c_void_p), reg.ctypes.data_as(C.c_void_p), 5, FW, FH, 3, C.c_double(0.05),
                                    out.ctypes.data_as(C.c_void_p), 4)
    assert rc == _lib.HP_ERR_CAPACITY and out.tobytes() == hs[:4].tobytes()
