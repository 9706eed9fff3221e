"""GPU: the engine's call side - from hp_engine_infer_u8 / hp_engine_infer_f32 to the replay of a captured graph, and the cache of captured
graphs in between (csrc/graph_cache.hpp; tests/cpp/graph_cache.cpp holds the cache alone to its rules on the host).

The engines are the smallest that have every launch kind of the call path: a first conv 3 -> 32, a 3 x 3 conv 32 -> 32 and a 1 x 1 head with
an fp32 output, on frames of 12 x 16, max_batch 4 (3 where the halves are 2 + 1): f32 with concurrency 1 and 2, f32s with concurrency 2,
f16 and i8 on one stream.  The flip-ensemble cases run tests/test_flip_engine_gpu.py's engine (lw_openpose_vggtiny at 88 x 56, COCO tables).

Expected values never come from the graph path.  Every buffer holds its own frames (seed = buffer index) and a TWIN engine - the same weights,
set_graph(False), concurrency 1 - runs every buffer once: one table of outputs per (buffer, frame) for the u8 entry, one for the f32 entry and
one with the ensemble on.  A frame's outputs do not depend on the batch it ran in (BATCH_DEPENDENT is empty in test_engine_tiny_maps_gpu.py), so
the tables serve every n, and every call of every test is compared with them bit for bit: a replay that reads a stale or wrong pointer
returns another buffer's maps.  The tables themselves are pinned to the torch fp32 oracle (oracle/ref_net.py) with the families' own
tolerances, unchanged: _close32 (fp32 engines), _close against the fp16-matched oracle (fp16), the int8 family's gate (no further from fp32
than the emulated quantization contract, 1.5 x + 1e-2); the ensemble table to hp_flip_merge_host of the plain outputs.

After every call hp_engine_cached_graphs is compared with a restatement of the key rule (`CacheModel`: which keys a call has, eviction when
the missing ones do not fit in 64), so the bound, the points of eviction and what a setting drops are all pinned.
"""
import ctypes as C
import functools
import types

import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import frontend, synth
from hyperpose_amd._lib import DevBuf, check, lib
from oracle import ref_net
from test_engine_fp32_gpu import _close32
from test_engine_gpu import Net, Out, _close
from test_engine_int8_gpu import _emulate_network, _rel
from test_flip_engine_gpu import MAX_BATCH as FLIP_BATCH
from test_flip_engine_gpu import NET_H, NET_W

pytestmark = pytest.mark.gpu

BOUND = 64
H, W = 12, 16
NBUF = 70
U8, F32 = 0, 1


class Rig:
    """One network at one size and dtype: `nbuf` buffers of max_batch frames each, on the host and as slices of one device allocation, and the
    twin's tables."""

    def __init__(self, layers, outputs, weights, h, w, max_batch, dtype, nbuf, frames, mean=(0, 0, 0), inv_std=(1, 1, 1), coco=False):
        self.layers, self.outputs, self.weights, self.h, self.w, self.mb, self.dtype, self.nbuf = layers, outputs, weights, h, w, max_batch, dtype, nbuf
        self.mean, self.inv_std, self.coco = mean, inv_std, coco
        self.halves_ok = dtype in ("f32", "f32s")
        self.frames = frames                                                               # [nbuf][mb, h, w, 3] u8
        self.frames32 = [np.random.default_rng(1000 + b).normal(size=(max_batch, 3, h, w)).astype(np.float32) for b in range(nbuf)]
        self.stride = max_batch * h * w * 3
        self.pool = DevBuf.from_numpy(np.concatenate(frames))
        self.scales = None
        if dtype == "i8":
            e = self._create()
            e.calibrate(np.concatenate(frames[:2]))
            self.scales = e.int8_scales
            e.close()
            assert (self.scales > 0).any(), "no layer of the net runs on the int8 pipe"
        twin = self.engine(1, graph=False)
        self.names = [o[0] for o in twin.outputs]
        self.plain = [self._stack(twin.inference(f)) for f in self.frames]
        self.plain32 = [self._stack(twin.inference_f32(f)) for f in self.frames32]
        self.flipped = None
        if coco:
            conf_perm, paf_perm, paf_sign = frontend.flip_tables_coco(twin.outputs[0][1][0])
            tabs = [(conf_perm, np.ones(conf_perm.size, np.int8)), (paf_perm, paf_sign)]
            k = max_batch // 2
            both = [self._stack(twin.inference(np.concatenate([f[:k], frontend.hflip_u8c3_host(f[:k])]))) for f in self.frames]
            twin.set_flip_ensemble(True)
            self.flipped = [self._stack(twin.inference(f[:k])) for f in self.frames]
            for b in range(nbuf):  # the ensemble table is the host merge of the plain outputs on [frames, flipped frames]
                for got, maps, (perm, sign) in zip(self.flipped[b], both[b], tabs):
                    assert got.tobytes() == frontend.flip_merge_host(maps, k, perm, sign)[:k].tobytes(), f"buffer {b}: ensemble != host merge"
        assert twin.split_fallbacks == 0
        twin.close()
        self._pin_to_the_oracle()

    @staticmethod
    def _stack(per_image):
        return [np.stack([img[i][1] for img in per_image]) for i in range(len(per_image[0]))]

    def _pin_to_the_oracle(self):
        """The twin's tables against oracle/ref_net.py, with the tolerance of the dtype's family."""
        kw = dict(mean=self.mean, inv_std=self.inv_std)
        for table, arg, src in ((self.plain, "frames_u8", self.frames), (self.plain32, "frames_f32", self.frames32)):
            x = np.concatenate(src)
            got = {nm: np.concatenate([t[i] for t in table]) for i, nm in enumerate(self.names)}
            ref = ref_net.run(self.layers, self.outputs, self.weights, match_fp16=self.dtype == "f16", **{arg: x}, **kw)
            assert sorted(ref) == self.names
            if self.dtype == "i8":
                if arg == "frames_f32":
                    continue  # (the family's emulation is of u8 frames)
                fp32 = ref_net.run(self.layers, self.outputs, self.weights, match_fp16=False, **{arg: x}, **kw)
                net = types.SimpleNamespace(layers=self.layers, outputs=self.outputs, mean=self.mean, inv_std=self.inv_std)
                emu = _emulate_network(net, self.weights, x, self.scales, pytest.MonkeyPatch())
                assert _rel(got, fp32) <= 1.5 * _rel(emu, fp32) + 1e-2
                continue
            for nm in self.names:
                for f in range(len(x)):
                    if self.dtype == "f16":
                        _close(got[nm][f], ref[nm][f])
                    else:
                        _close32(got[nm][f], ref[nm][f], f"{nm} of frame {f}")

    def _create(self):
        return E.Engine(self.layers, self.outputs, self.weights, self.w, self.h, self.mb, mean=self.mean, inv_std=self.inv_std, dtype=self.dtype)

    def engine(self, parts, graph=True):
        e = self._create()
        if self.scales is not None:
            e.int8_scales = self.scales
        e.set_graph(graph)
        e.set_concurrency(parts)
        assert e.concurrency == (parts if self.halves_ok else 1) and e.cached_graphs == 0
        return e

    def ptr(self, b):
        return self.pool.ptr.value + b * self.stride

    def want(self, b, n, kind=U8, flip=False):
        return [t[:n] for t in (self.flipped if flip else self.plain32 if kind == F32 else self.plain)[b]]


def _tiny(dtype, max_batch=4):
    return _tiny_rig(dtype, max_batch)


@functools.lru_cache(maxsize=None)
def _tiny_rig(dtype, max_batch):
    net = Net(41)
    t = net.conv(0, 3, 32, 3, 1)
    t = net.conv(t, 32, 32, 3, 1)
    t = net.conv(t, 32, 6, 1, act=E.ACT_NONE)
    frames = [np.random.default_rng(b).integers(0, 256, (max_batch, H, W, 3), dtype=np.uint8) for b in range(NBUF)]
    return Rig(net.layers, [Out("y", t, 0, 6).c()], net.blob(), H, W, max_batch, dtype, NBUF, frames)


VGG_NBUF = 40


@functools.lru_cache(maxsize=None)
def _vgg():
    m = E.Model("lw_openpose_vggtiny", NET_W, NET_H)
    frames = [synth.images_u8(synth.rng_for(b, salt=71), FLIP_BATCH, NET_H, NET_W) for b in range(VGG_NBUF)]
    rig = Rig(m.layers, m.outputs, m.init_weights(5), NET_H, NET_W, FLIP_BATCH, "f32", VGG_NBUF, frames, m.mean, m.inv_std, coco=True)
    rig.model = m  # (the layer and output arrays point into it)
    return rig


@functools.lru_cache(maxsize=None)
def _caller_streams():
    """Two streams that are not the engine's: those of two other engines.  Waiting for such a stream is hp_engine_synchronize of its owner."""
    return _tiny("f16").engine(1), _tiny("f16").engine(1)


class CacheModel:
    """Which keys a call has (infer_common) and when the cache is emptied (graph_cache.hpp), restated: (frames, pointer, kind, first frame);
    a host batch is keyed by the staging buffer; with the ensemble on by the caller's pointer (one stream, device batch) or the engine's
    flip buffer; eviction of everything when the call's missing keys do not fit."""

    def __init__(self, rig, parts):
        self.rig, self.parts, self.flip, self.graph, self.keys, self.evictions = rig, parts if rig.halves_ok else 1, False, True, set(), 0

    def call(self, kind, ptr, n, on_device):
        if not self.graph:
            return
        dev, src = (ptr if on_device else "stage"), None
        if self.flip:
            dev, src, n, kind = "flip_in", (ptr if on_device else None), 2 * n, 2
        halves = self.parts == 2 and n >= 2
        p = src if src is not None and not halves else dev
        n0 = (n + 1) // 2
        keys = [(n0, p, kind, 0), (n - n0, p, kind, n0)] if halves else [(n, p, kind, 0)]
        missing = sum(k not in self.keys for k in keys)
        if missing and len(self.keys) + missing > BOUND:
            self.keys.clear()
            self.evictions += 1
        self.keys.update(keys)

    def drop(self):
        self.keys.clear()


class Driver:
    """An engine, its cache model and the streams: call, wait on the call's stream, read the outputs from the device, compare."""

    def __init__(self, rig, parts):
        self.rig, self.eng, self.model = rig, rig.engine(parts), CacheModel(rig, parts)
        a, b = _caller_streams()
        self.owners = {"own": self.eng, "A": a, "B": b}
        self.fell = 0      # times cached_graphs fell below its value after the previous call (no setting changed in between)
        self.prev = 0

    def close(self):
        assert self.eng.split_fallbacks == 0
        self.eng.close()

    def enqueue(self, b, n, kind=U8, on_device=True, stream="own", at=None):
        rig = self.rig
        if on_device:
            src = C.c_void_p(rig.ptr(b) if at is None else at)  # (`at`: another device address that holds the frames)
            key_ptr = src.value
        else:
            self.host = np.ascontiguousarray((rig.frames32 if kind == F32 else rig.frames)[b][:n])  # kept alive until the call has run
            src, key_ptr = self.host.ctypes.data_as(C.c_void_p), None
        fn = lib().hp_engine_infer_f32 if kind == F32 else lib().hp_engine_infer_u8
        check(fn(self.eng._h, src, int(n), int(on_device), None if stream == "own" else C.c_void_p(self.owners[stream].stream)))
        self.model.call(kind, key_ptr, n, on_device)
        c = self.eng.cached_graphs
        assert c <= BOUND and c == len(self.model.keys), f"{c} cached graphs, by the key rule {len(self.model.keys)}"
        self.fell += c < self.prev
        self.prev = c

    def read(self, n, stream="own"):
        self.owners[stream].synchronize()  # the caller's stream alone: the second half has joined it
        out = []
        for _, shape, dev in self.eng.outputs:
            a = np.empty((n,) + shape, np.float32)
            check(lib().hp_memcpy_d2h(a.ctypes.data_as(C.c_void_p), C.c_void_p(dev), C.c_size_t(a.nbytes)))
            out.append(a)
        return out

    def run(self, b, n, kind=U8, on_device=True, stream="own", what=""):
        self.enqueue(b, n, kind, on_device, stream)
        self.same(self.read(n, stream), self.rig.want(b, n, kind, self.model.flip), f"{what}buffer {b}, {n} frames, kind {kind}, device {on_device}, stream {stream}")

    def same(self, got, want, what):
        for nm, g, w_ in zip(self.rig.names, got, want):
            assert g.shape == w_.shape and g.tobytes() == w_.tobytes(), f"{what}: output {nm} is not the twin's"

    # ---- settings
    def after_setting(self, dropped):
        if dropped:
            self.model.drop()
        assert self.eng.cached_graphs == len(self.model.keys), f"{self.eng.cached_graphs} cached graphs after a setting, expected {len(self.model.keys)}"
        self.prev = self.eng.cached_graphs

    def set_concurrency(self, parts):
        self.eng.set_concurrency(parts)
        parts = parts if self.rig.halves_ok else 1
        changed, self.model.parts = parts != self.model.parts, parts
        assert self.eng.concurrency == parts
        self.after_setting(changed)
        assert not changed or self.eng.cached_graphs == 0

    def set_flip(self, on):
        self.eng.set_flip_ensemble(on)
        self.model.flip = on
        self.after_setting(True)
        assert self.eng.cached_graphs == 0 and self.eng.flip_ensemble == on

    def set_graph(self, on):
        self.eng.set_graph(on)
        self.model.graph = on
        self.after_setting(False)

    def set_same_int8_scales(self):
        self.eng.int8_scales = self.eng.int8_scales
        self.after_setting(True)
        assert self.eng.cached_graphs == 0


# (dtype, concurrency, max_batch): max_batch 3 runs the full batch as halves of 2 + 1
ENGINES = [("f32", 1, 4), ("f32", 2, 4), ("f32", 2, 3), ("f32s", 2, 4), ("f16", 1, 4), ("i8", 1, 4)]
IDS = [f"{d}-c{p}-b{m}" for d, p, m in ENGINES]


@pytest.mark.parametrize("dtype,parts,mb", ENGINES, ids=IDS)
def test_more_buffers_than_the_cache_holds(hp, dtype, parts, mb):
    """70 device pointers, each with a full batch, 2 frames and 1 frame, twice round.  (With concurrency 2 the 2-frame call's first half and
    the 1-frame call share a key; a pointer has 4 keys, so the cache is emptied about every 16 pointers and every key is captured again.)"""
    d = Driver(_tiny(dtype, mb), parts)
    try:
        for rnd in range(2):
            for b in range(NBUF):
                for n in (mb, 2, 1):
                    d.run(b, n, what=f"round {rnd}: ")
        assert d.fell >= 1 and d.model.evictions >= 2, "the run never reached eviction"
    finally:
        d.close()


@pytest.mark.parametrize("dtype,parts", [("f32", 2), ("f16", 1)])
def test_same_pointer_new_content(hp, dtype, parts):
    rig = _tiny(dtype)
    d = Driver(rig, parts)
    mine = DevBuf(rig.stride)
    try:
        for n in (4, 1, 3):
            for step, b in enumerate((3, 8, 3, 21)):
                check(lib().hp_memcpy_h2d(mine.ptr, rig.frames[b].ctypes.data_as(C.c_void_p), C.c_size_t(rig.stride)))
                before = d.eng.cached_graphs
                d.enqueue(b, n, at=mine.ptr.value)
                d.same(d.read(n), rig.want(b, n), f"device buffer rewritten with buffer {b}'s frames, {n} frames")
                assert step == 0 or d.eng.cached_graphs == before
        cached = d.eng.cached_graphs
        for n in (4, 2):  # the host entry: the staging buffer is the key
            for step, b in enumerate((5, 6, 5)):
                before = d.eng.cached_graphs
                d.run(b, n, on_device=False)
                assert step == 0 or d.eng.cached_graphs == before
            for step, b in enumerate((7, 9)):
                before = d.eng.cached_graphs
                d.run(b, n, kind=F32, on_device=False)
                assert step == 0 or d.eng.cached_graphs == before
        assert d.eng.cached_graphs == cached + (4 if parts == 1 else 8)  # per n: one u8 and one f32 key, or their two halves
    finally:
        d.close()
        mine.free()


@pytest.mark.parametrize("mb", [4, 3])
@pytest.mark.parametrize("order", [(2, 1), (1, 2)])
def test_two_frames_and_one_frame_on_one_pointer(hp, mb, order):
    """Concurrency 2: the 1-frame call's key is the key of the 2-frame call's first half."""
    d = Driver(_tiny("f32", mb), 2)
    try:
        for b in (0, 1):
            for i, n in enumerate(order + order):
                d.run(b, n)
                assert d.eng.cached_graphs == 2 * b + (2 if n == 2 or i >= 1 else 1)
        d.run(0, mb)
        assert d.eng.cached_graphs == 6
    finally:
        d.close()


@pytest.mark.parametrize("dtype,parts", [("f32", 2), ("f16", 1)])
def test_u8_and_f32_entries_alternate_on_one_address(hp, dtype, parts):
    rig = _tiny(dtype)
    d = Driver(rig, parts)
    mine = DevBuf(rig.frames32[0].nbytes)  # room for either kind of batch
    try:
        for b, n in ((0, 4), (1, 2), (2, 4), (3, 1), (4, 3), (0, 4)):
            for kind, src in ((U8, rig.frames[b]), (F32, rig.frames32[b]), (U8, rig.frames[b + 10])):
                check(lib().hp_memcpy_h2d(mine.ptr, src.ctypes.data_as(C.c_void_p), C.c_size_t(src.nbytes)))
                d.enqueue(b, n, kind=kind, at=mine.ptr.value)
                d.same(d.read(n), rig.want(b + 10 if src is rig.frames[b + 10] else b, n, kind), f"buffer {b}, {n} frames, kind {kind} at one address")
        assert len({k[2] for k in d.model.keys}) == 2 and len({k[1] for k in d.model.keys}) == 1
    finally:
        d.close()
        mine.free()


@pytest.mark.parametrize("dtype", ["f32", "f32s"])
def test_caller_streams(hp, dtype):
    """Calls alternately on the engine's stream and two caller streams; after each the test waits for that stream alone and reads.  Then an
    eviction and two set_concurrency changes happen while the call before them, on the OTHER caller stream, has not been waited for."""
    rig = _tiny(dtype)
    d = Driver(rig, 2)
    order = ("own", "A", "B")
    try:
        for i in range(30):
            d.run(i, 1 + i % rig.mb, stream=order[i % 3])
        b = 30
        while len(d.model.keys) < BOUND:  # one-frame calls: one key each, up to the bound exactly
            d.run(b, 1, stream=order[b % 3])
            b += 1
        assert d.eng.cached_graphs == BOUND and b < NBUF - 1 and d.model.evictions == 0
        d.enqueue(0, 1, stream="A")            # cached; in flight on A, not waited for
        d.enqueue(NBUF - 1, rig.mb, stream="B")  # two new keys: everything cached is destroyed first
        assert d.model.evictions == 1 and d.eng.cached_graphs == 2 and d.fell == 1
        d.same(d.read(rig.mb, "B"), rig.want(NBUF - 1, rig.mb), "the call that evicted, on stream B")
        d.enqueue(NBUF - 1, rig.mb, stream="B")  # cached; in flight on B, not waited for
        d.set_concurrency(1)
        d.run(5, rig.mb, stream="A")
        d.run(NBUF - 1, 2, stream="own")
        d.enqueue(5, rig.mb, stream="A")       # in flight on A
        d.set_concurrency(2)
        d.run(6, rig.mb, stream="B")
        d.run(5, rig.mb, stream="own")
    finally:
        d.close()


def test_settings_with_a_warm_cache(hp):
    """lw_openpose_vggtiny, fp32: every setting that changes the schedule empties the cache, set_graph keeps it, and the next calls on old and
    new pointers are the twin's for the setting in force."""
    rig = _vgg()
    d = Driver(rig, 1)

    def warm():
        for b in range(10):
            d.run(b, rig.mb if not d.model.flip else rig.mb // 2)
        assert d.eng.cached_graphs >= 10 or d.model.flip

    def old_and_new(what):
        k = rig.mb // 2 if d.model.flip else rig.mb
        for b, n in ((3, k), (12, k - 1 or 1), (3, 1), (13, k)):
            d.run(b, n, what=what)
        d.run(4, k, on_device=False, what=what)

    try:
        warm()
        d.set_concurrency(2)
        old_and_new("concurrency 1 -> 2: ")
        warm()
        d.set_concurrency(1)
        old_and_new("concurrency 2 -> 1: ")
        warm()
        d.set_flip(True)
        old_and_new("ensemble on: ")
        warm()
        d.set_concurrency(2)
        old_and_new("ensemble on, concurrency 2: ")
        d.set_flip(False)
        old_and_new("ensemble off: ")
        warm()
        cached = d.eng.cached_graphs
        d.set_graph(False)
        assert d.eng.cached_graphs == cached
        old_and_new("captured graphs off: ")
        assert d.eng.cached_graphs == cached
        d.set_graph(True)
        assert d.eng.cached_graphs == cached
        d.run(3, rig.mb, what="captured graphs on again: ")
        assert d.eng.cached_graphs == cached
        old_and_new("captured graphs on again: ")
    finally:
        d.close()


def test_int8_scales_with_a_warm_cache(hp):
    rig = _tiny("i8")
    d = Driver(rig, 1)
    try:
        for b in range(10):
            d.run(b, rig.mb)
        assert d.eng.cached_graphs == 10
        d.set_same_int8_scales()
        for b, n in ((3, 4), (12, 3), (3, 1), (13, 4)):
            d.run(b, n, what="int8 scales set again: ")
        d.set_graph(False)
        d.run(3, 4)
        d.set_graph(True)
        assert d.eng.cached_graphs == 4
        d.run(3, 4)
    finally:
        d.close()


@pytest.mark.parametrize("which,parts,calls", [("f32", 2, 200), ("f16", 1, 200), ("vgg", 2, 180)])
def test_seeded_mixed_sequence(hp, which, parts, calls):
    """Buffer, n, entry (u8 device 80 %, u8 host, f32 host), stream (own, A, B) drawn per call; from call 90 on, now and then a setting
    changes: concurrency, captured graphs off / on, and on the COCO engine the ensemble."""
    seed = 20240 + parts + calls
    rng = np.random.default_rng(seed)
    rig = _vgg() if which == "vgg" else _tiny(which)
    d = Driver(rig, parts)
    settings = ["concurrency", "graph"] + (["flip", "flip"] if rig.coco else [])
    i = -1
    try:
        for i in range(calls):
            if i >= 90 and rng.random() < 0.08:
                s = settings[int(rng.integers(len(settings)))]
                if s == "concurrency":
                    d.set_concurrency(3 - d.model.parts if rig.halves_ok else 2)
                elif s == "graph":
                    d.set_graph(not d.model.graph)
                else:
                    d.set_flip(not d.model.flip)
            b = int(rng.integers(rig.nbuf))
            n = 1 + int(rng.integers(rig.mb // 2 if d.model.flip else rig.mb))
            entry = int(rng.choice(3, p=[0.8, 0.1, 0.1]))
            if d.model.flip and entry == 2:
                entry = 1  # (the ensemble is defined on u8 frames)
            stream = ("own", "A", "B")[int(rng.integers(3))]
            d.run(b, n, kind=F32 if entry == 2 else U8, on_device=entry == 0, stream=stream)
        assert d.fell >= 1 and d.model.evictions >= 1, "the sequence never reached eviction"
    except BaseException:
        print(f"\ntest_seeded_mixed_sequence[{which}]: seed {seed}, call {i}")
        raise
    finally:
        d.close()
