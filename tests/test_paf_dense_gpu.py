"""GPU: the PAF parser on DENSE maps (hundreds of maxima per part, tens of thousands of candidate pairs per limb, more than a thousand
connections per frame) against the reference-compiled oracle, bit for bit - the regime of a network's own maps under random weights.

What is under test: paf_score_kernel's cut of a frame's pair index space into tiles dealt out to its blocks (tiles that end inside a limb,
limbs that span many tiles and blocks, blocks that cross from one limb to the next, empty limbs and frames next to them), the candidate
lists in device memory whose arrival order must not show in any result, their counters between batches (paf_connect_kernel leaves them zero, also after a re-parse with doubled lists), ties through paf_connect_kernel, and
paf_assemble_kernel's whole-limb-in-parallel path on its LDS tables (frames with more than 64 skeleton fragments).

Every test asserts, from the ORACLE's result, the property it exists for.
"""
import functools

import numpy as np
import pytest

from hyperpose_amd import synth
from oracle import loader

pytestmark = pytest.mark.gpu

ROWS, COLS = 46, 54
CAPS = dict(cap_humans=1024, cap_peaks=65536, cap_conns=65536)
COCOPAIRS = ((1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (1, 8), (8, 9), (9, 10), (1, 11), (11, 12), (12, 13), (1, 0), (0, 14), (14, 16),
             (0, 15), (15, 17), (2, 16), (5, 17))


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _dense(seed, rows=ROWS, cols=COLS):
    """i.i.d. maps: conf = U[0, 0.12), paf = N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 0.12, (19, rows, cols)).astype(np.float32), rng.normal(0, 0.3, (38, rows, cols)).astype(np.float32)


def _people(salt, people, rows=ROWS, cols=COLS, **kw):
    conf, paf, _ = synth.paf_maps(synth.rng_for(1, salt=salt), len(people), rows, cols, people=people, **kw)
    return [(conf[i], paf[i]) for i in range(len(people))]


def _candidate_overflow():
    """The forced-overflow frame of test_paf_gpu.py::test_lists_grow_like_the_references_vectors: 66 necks left, 66 right shoulders right,
    a constant PAF pointing right -> thousands of the 4356 pairs of limb 0 pass both criteria (the initial list holds 2048)."""
    conf = np.zeros((19, ROWS, COLS), np.float32)
    paf = np.zeros((38, ROWS, COLS), np.float32)
    yy, xx = np.mgrid[0:ROWS, 0:COLS].astype(np.float32)
    for gy in range(2, ROWS - 1, 4):
        for gx in range(1, COLS // 2 - 2, 4):
            conf[1] += np.exp(-((xx - gx) ** 2 + (yy - gy) ** 2) / 0.5).astype(np.float32)
            conf[2] += np.exp(-((xx - (gx + COLS // 2)) ** 2 + (yy - gy) ** 2) / 0.5).astype(np.float32)
    paf[12] = 1.0
    conf[18] = 1 - conf[:18].max(0)
    return conf, paf


def _tie_maps(n_necks, rows=ROWS, cols=COLS, gap=4):
    """test_paf_gpu.py::_tie_maps: candidate connections of limb 0 that TIE exactly - every neck has a shoulder `gap` cells to its right and
    one `gap` cells to its left, the PAF x-field is exactly +1 right of the neck column and -1 left of it; the two tied candidates share
    the neck, so which one survives get_connections' greedy pass is decided by the sort order of equal scores."""
    conf = np.zeros((19, rows, cols), np.float32)
    paf = np.zeros((38, rows, cols), np.float32)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float32)

    def blob(k, y, x, a=1.0):
        conf[k] += a * np.exp(-((xx - x) ** 2 + (yy - y) ** 2) / 2.0).astype(np.float32)
    cx = cols // 2
    for y in np.linspace(4, rows - 5, n_necks).astype(int):
        blob(1, y, cx)
        blob(2, y, cx + gap)
        blob(2, y, cx - gap)
    paf[12][:, cx + 1:] = 1.0
    paf[12][:, :cx] = -1.0
    conf[18] = 1 - conf[:18].max(0)
    return conf, paf


@functools.lru_cache(maxsize=None)
def frames(name):
    """The named input frames of this file, each built once: (conf [19, R, C], paf [38, R, C])."""
    if name.startswith("dense"):          # dense0, dense1, dense2: 46 x 54
        return _dense(9100 + int(name[5:]))
    if name.startswith("small"):          # small0 .. small2: 16 x 20
        return _dense(9200 + int(name[5:]), 16, 20)
    if name == "odd":                     # 13 x 70: odd sizes, two strips of the peaks kernel
        return _dense(9300, 13, 70)
    if name == "zero":
        return np.zeros((19, ROWS, COLS), np.float32), np.zeros((38, ROWS, COLS), np.float32)
    if name == "people6":
        return _people(81, (6,))[0]
    if name.startswith("sparse"):         # sparse0 .. sparse3
        return _people(82, (3, 7, 1, 5))[int(name[6:])]
    if name == "crowd":                   # test_random_crowds_against_oracle's generator: 30 people on noisy maps
        conf, paf, _ = synth.paf_maps(np.random.default_rng(77 + 9), 1, people=(30,), noise=0.06, drop_joint_prob=0.05)
        return conf[0], paf[0]
    if name == "overflow":
        return _candidate_overflow()
    if name == "ties":
        return _tie_maps(12, gap=4)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(humans, peaks, connections) of the reference's parser on frames(name), computed once and shared."""
    conf, paf = frames(name)
    return loader.ref_paf_process(conf, paf, **CAPS)


def _batch(names):
    return np.stack([frames(n)[0] for n in names]), np.stack([frames(n)[1] for n in names])


def _run_and_check(parser, names):
    conf, paf = _batch(names)
    humans = parser.process_batch(conf, paf)
    for f, n in enumerate(names):
        oh, op, oc = oracle(n)
        gp = parser.debug_peaks(f, cap=65536)
        assert _same(gp, op), f"{n}: peaks differ: gpu {len(gp)} vs oracle {len(op)}"
        gc = parser.debug_conns(f, cap=65536)
        assert _same(gc, oc), f"{n}: connections differ: gpu {len(gc)} vs oracle {len(oc)}"
        assert _same(humans[f], oh), f"{n}: humans differ: gpu {len(humans[f])} vs oracle {len(oh)}"
    return humans


def _pairs_per_limb(peaks):
    cnt = np.bincount(peaks["part_id"], minlength=18)
    return [int(cnt[a]) * int(cnt[b]) for a, b in COCOPAIRS]


def _parser(max_batch):
    from hyperpose_amd.parser import Paf
    return Paf(max_batch=max_batch, cap_per_frame=256)


MIXED = ("dense0", "zero", "people6", "dense1")


def test_limbs_span_many_tiles_next_to_empty_and_sparse_frames(hp):
    """A limb of the dense frame is more than 8 tiles of the scoring kernel (16 384 pairs), the all-zero frame next to it has no pair at
    all (every scoring block of that frame leaves at once), the frame with people has limbs of a few pairs: tiles straddle limbs and frames."""
    assert max(_pairs_per_limb(oracle("dense0")[1])) > 16384
    assert len(oracle("zero")[1]) == 0
    assert len(oracle("people6")[0]) >= 1
    _run_and_check(_parser(4), MIXED)


def test_small_geometries_tiles_end_inside_a_limb(hp):
    pairs = [p for i in range(3) for p in _pairs_per_limb(oracle(f"small{i}")[1])]
    assert min(pairs) > 512 and all(p % 512 for p in pairs)    # every limb: more than one tile of 512 pairs, the last one partial
    assert sum(len(oracle(f"small{i}")[2]) for i in range(3)) > 100
    _run_and_check(_parser(3), ("small0", "small1", "small2"))
    assert len(oracle("odd")[2]) > 0
    _run_and_check(_parser(1), ("odd",))


def test_arrival_order_does_not_leak(hp):
    """The candidates of a limb reach their list in whatever order the scoring blocks get to its counter: three runs of the same batch
    through one parser give the same bytes (and the oracle's)."""
    p = _parser(4)
    conf, paf = _batch(MIXED)
    assert max(_pairs_per_limb(oracle("dense1")[1])) > 16384
    runs = []
    for _ in range(3):
        humans = p.process_batch(conf, paf)
        runs.append(([h.copy() for h in humans], [p.debug_conns(f, cap=65536) for f in range(4)]))
    for humans, conns in runs:
        for f, n in enumerate(MIXED):
            assert _same(humans[f], runs[0][0][f]) and _same(conns[f], runs[0][1][f]), n
            assert _same(humans[f], oracle(n)[0]) and _same(conns[f], oracle(n)[2]), n


def test_candidate_counters_between_batches(hp):
    """ONE parser: dense and sparse batches of different sizes, then a batch whose limb 0 overflows the candidate list (re-parsed with
    doubled lists inside collect), then a sparse batch again: the connect kernel leaves every candidate counter zero, also after a re-parse."""
    p = _parser(4)
    _run_and_check(p, MIXED)
    _run_and_check(p, ("sparse0", "sparse1"))
    _run_and_check(p, ("dense2",))
    _run_and_check(p, ("sparse0", "sparse1", "sparse2", "sparse3"))
    oc = oracle("overflow")[2]
    assert len(oc[oc["pair_id"] == 0]) >= 66
    _run_and_check(p, ("overflow", "sparse2"))
    _run_and_check(p, ("sparse3", "sparse0", "sparse1"))


def test_assembly_beyond_64_fragments(hp):
    """The assembly kernel's walk on its LDS tables: limbs that go 64 connections per step (nothing held at the limb's second part, no
    peak held twice at its first) and limbs that keep the sequential walk (the last two limbs revisit parts 16 / 17)."""
    _, op, oc = oracle("dense0")
    assert len(oc) > 512
    # every connection of limb 0 opens a skeleton fragment, and so does every connection of limb 1 whose neck limb 0 did not use
    l0, l1 = oc[oc["pair_id"] == 0], oc[oc["pair_id"] == 1]
    assert len(l0) + int(np.sum(~np.isin(l1["cid1"], l0["cid1"]))) > 64
    assert min(int(np.sum(oc["pair_id"] == l)) for l in range(19)) > 0      # the two limbs that never qualify included
    ch, _, cc = oracle("crowd")
    assert len(ch) >= 10 and int(np.sum(cc["pair_id"] >= 17)) > 0
    _run_and_check(_parser(2), ("dense0", "crowd"))


def test_ties_through_the_connect_kernel(hp):
    """24-way ties among more than 16 candidates (libstdc++'s introsort decides their order) next to a dense frame."""
    oh, op, oc = oracle("ties")
    limb0 = oc[oc["pair_id"] == 0]
    assert len(limb0) == 12                                 # one survivor per neck: the ties really conflicted
    assert np.all(limb0["score"] == limb0["score"][0])      # ... and really were exact ties
    _run_and_check(_parser(2), ("dense1", "ties"))
    _run_and_check(_parser(2), ("ties", "dense1"))
