"""GPU: every convolution kernel family on maps SMALLER than its tile and its window.

hp_engine_create takes any input size, and the built-in topologies at 32 x 32 already hand 1 x 1 maps to ResNet-50's last stage.  Every
kernel is written around a tile (16 x 12, 8 x 12, 4 x 8 pixels, 64 / 128 pixels of the whole batch, 2 x 2 Winograd tiles, column pairs);
test_engine_footprint_gpu.py stops one pixel below a tile.  Here the same catalogue of graphs (CASES: one per family and variant, with
its forcing environment, a consumer that gives the tested tensor a halo, and a predicate on the profile's tile code) runs on frames of
1 x 1, 1 x 7, 5 x 1, 2 x 2, 3 x 4 and 4 x 3 pixels at batch 3: a 7 x 7 or dilation-2 window that is mostly padding, a halo tile larger than
the image, a GEMM tile that holds all images at once, a Winograd tile / depthwise column pair whose second row or column does not exist,
a 3/2 pool window with one real element, a bilinear up-sample from one pixel, and halo / separator-row / pad-channel writes around a map
whose halo is larger than its interior.  Tolerances are the families' own (_close with the case's `tol`, _close32), unchanged.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import footprint
from hyperpose_amd import engine as E
from oracle import ref_net
from test_engine_footprint_gpu import ARCHS, CASES, _make, _set_env, _values, generic16, guarded, tile_at
from test_engine_fp32_gpu import _close32
from test_engine_gpu import Net, Out, _check, _close, _frames
from test_engine_int8_gpu import _emulate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
N = 3
TINY = [(1, 1), (1, 7), (5, 1), (2, 2), (3, 4), (4, 3)]      # (h, w) of the frame = of the tested layer's input: the stems are stride 1
BY_NAME = {c.name: c for c in CASES}

# Cases whose own kernel does not serve maps this small: {case name: (predicate on the profile rows that must hold instead, reason)}.
ROUTED_AWAY = {
    # conv_pick.hpp:58 (use_gdirect): a 3 x 3 layer leaves conv_direct_kernel where its 16 x 12 tiles cover less than 68 % of their
    # pixels - 1 .. 12 of 192 here; conv3x3_direct_kernel (use_halo, conv_pick.hpp:69) has no 256- / 512-channel form, so pick_conv(p, 1)
    # is not ok, conv_weight_layout answers 0 and the layer runs on conv_mfma_kernel.  No split, so `differs_from` does not apply.
    "f16-direct-3x3-splitk": (tile_at(1, lambda r: generic16(r["tile"])), "conv_pick.hpp:58 then :69: 3 x 3 on 256 channels -> conv_mfma_kernel"),
    "f16-direct-3x3-splitk4": (tile_at(1, lambda r: generic16(r["tile"])), "conv_pick.hpp:58 then :69: 3 x 3 on 512 channels -> conv_mfma_kernel"),
    # conv_pick.hpp:91 (big1x1_variant): <2, 2> needs >= 320 blocks of 64 pixels x 256 channels, conv_pick.hpp:95-96 <1, 4> >= 1024 blocks of
    # 128 pixels x 128 channels; 3 .. 36 pixels are one block per channel group: conv1x1_big_kernel<1, 2>
    "f16-big1x1-1024-residual-2x2": (tile_at(2, lambda r: r["tile"] == 5201002), "conv_pick.hpp:91: fewer than 320 blocks -> conv1x1_big_kernel<1, 2>"),
    "f16-big1x1-640-1x4": (tile_at(1, lambda r: r["tile"] == 5201002), "conv_pick.hpp:96: fewer than 1024 blocks -> conv1x1_big_kernel<1, 2>"),
}
# Cases whose summation order may depend on the batch size: {case name: source line and reason}.  None: every family sums a pixel's
# products in an order that the other pixels of its tile do not change.
BATCH_DEPENDENT = {}
# The dense fp16 layers: launch_conv_mfma runs what pick_conv (csrc/conv_pick.hpp) says; the expected tile code comes from that text in a
# host program of its own (tests/cpp/conv_pick_at.cpp), not from the engine.
DENSE16 = ("f16-mfma-", "f16-small1x1-", "f16-big1x1", "f16-conv3x3-direct-", "f16-direct-")
assert len(BY_NAME) == len(CASES) and set(ROUTED_AWAY) <= set(BY_NAME) and set(BATCH_DEPENDENT) <= set(BY_NAME)

# Winograd F(2 x 2) on these maps, from launch_conv32_winograd (all forms report tile 35003004).  T = (OH + 1) / 2 <= 3 tile rows per image is
# below a block's 4 nc, so the ROWS form is never taken.  The input (the stem's output, P = 1) holds its images vh = H + 2 rounded up to
# even = 4, 4, 8, 4, 6, 6 rows apart (h = 1, 1, 5, 2, 3, 4), which winograd_tall accepts (vh even, >= H + 2):
#   nc = 2 (16-row blocks; "f32-winograd", "f32-winograd-residual-70ch"): tall_y = ceil((2 vh + H) / 16) = 1, 1, 2, 1, 1, 1 < 3 = one block row
#       per image: the TALL form at every size;
#   HP_WINO_NC=1 (8-row blocks; "f32-winograd-small-blocks"): tall_y = ceil((2 vh + H) / 8) = 2, 2, 3, 2, 2, 2: TALL at every size but 5 x 1,
#       where 3 is no fewer than the images' own 3 block rows: PER IMAGE;
#   HP_WINO_TALL=0 ("f32-winograd-per-image"): PER IMAGE at every size.


@pytest.fixture(scope="module")
def picker():
    """pick(layer, sizes) -> the tile code pick_conv gives the dense fp16 layer on each (h, w) at batch N."""
    src, exe = os.path.join(ROOT, "tests", "cpp", "conv_pick_at.cpp"), os.path.join(ROOT, "tests", "cpp", "conv_pick_at.bin")
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "include"), src, "-o", exe])

    def pick(L, sizes):
        assert L.op == E.OP_CONV and L.kh == L.kw
        args = [L.kh, L.cin, L.cout, N, L.stride, L.dil, int(L.res >= 0)] + [v for hw in sizes for v in hw]
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stdout + out.stderr
        tiles = [int(t) for t in out.stdout.split()]
        assert len(tiles) == len(sizes)
        return tiles
    return pick


def _bits(a):
    a = np.ascontiguousarray(a, np.float32)
    return a.view(np.uint32)


def _ulp_gate(got, want16, what):
    """test_engine_int8_gpu._fp16_gate's first half - the stored tensor is fp16 and within one fp16 ulp of the emulation everywhere - and
    the counts (bit-identical, all) of its second half, which the caller pools over the six sizes."""
    got16 = got.astype(np.float16)
    assert np.array_equal(got16.astype(np.float32), got), f"{what}: stored tensor is not fp16"
    ulp = np.spacing(np.abs(want16)).astype(np.float32)
    diff = np.abs(got16.astype(np.float32) - want16.astype(np.float32))
    assert (diff <= ulp).all(), f"{what}: max diff {diff.max():.4g} beyond one fp16 ulp"
    return int((got16.view(np.uint16) == want16.view(np.uint16)).sum()), got16.size


@pytest.mark.parametrize("name", list(BY_NAME))
@guarded
def test_family_on_tiny_maps(hp, monkeypatch, picker, name):
    """On every size of TINY: the tested tensor has a halo of >= 2 pixels around an interior of 1 .. 12 pixels (up-sampled: x 9); outputs and tested tensors
    match the oracle; everything outside every interior is zero after the inference and after the profiler's pass; the profile shows the
    family's kernel (or, for ROUTED_AWAY, the kernel named there); frame 2 alone gives the bits it gave inside the batch of three."""
    case = BY_NAME[name]
    _set_env(monkeypatch, case.env)
    f16 = case.dtype in ("f16", "i8")
    same = total = 0
    expected = None
    for si, (h, w) in enumerate(TINY):
        what = f"{name} {h}x{w}"
        net, tested, outs, eng = _make(case, h, w)
        frames = _frames(N, h, w, seed=h * 100 + w)
        ids = footprint.tensor_ids(net.layers)
        # a condition on the input: a kernel that writes zeros cannot pass
        tens = ref_net.run(net.layers, outs, net.blob(), frames_u8=frames, match_fp16=f16, return_tensors=True)[1]
        for t in tested:
            share = float(np.mean(tens[t] != 0))
            assert np.isfinite(tens[t]).all() and share >= 0.2, (what, t, share)
        got = eng.inference(frames)
        for t in tested:
            g = eng.debug_raw(t)[1]
            assert g["P"] >= 2 and g["max_batch"] == N, (what, g)
        assert footprint.assert_zero_outside(eng, ids, N, what) >= len(tested)
        if case.dtype == "i8":
            li = next(i for i, L in enumerate(net.layers) if L.out == tested[0])
            s = eng.int8_scales
            assert s[li] > 0
            v = _emulate(net.layers[li], eng.debug_tensor(net.layers[li].in_, N), net.blob(), s[li])
            a, b = _ulp_gate(eng.debug_tensor(tested[0], N), v.astype(np.float16), what)
            same, total = same + a, total + b
        else:
            _values(case, net, tested, outs, eng, got, frames, N)
        batch = [eng.debug_tensor(t, N) for t in tested]
        # ---- routing
        rows = eng.profile(N, 1)
        shown = [(r["layer"], r["op"], r["tile"]) for r in rows]
        if name in ROUTED_AWAY:
            assert ROUTED_AWAY[name][0](rows) and not case.want(rows), (what, ROUTED_AWAY[name][1], shown)
        else:
            assert case.want(rows), (what, shown)
        if name.startswith(DENSE16):
            li = next(i for i, L in enumerate(net.layers) if L.out == tested[0])
            if expected is None:
                expected = picker(net.layers[li], TINY)
            assert [r["tile"] for r in rows if r["layer"] == li] == [expected[si]], (what, expected[si], shown)
        assert footprint.assert_zero_outside(eng, ids, None, what + " after profile") >= len(tested)   # (the profiler runs every step again)
        # ---- batch invariance: on these maps one GEMM tile holds every image of the batch
        eng.inference(frames[2:3])
        assert footprint.assert_zero_outside(eng, ids, 1, what + " n=1") >= len(tested)
        if name not in BATCH_DEPENDENT:
            for t, full in zip(tested, batch):
                alone = eng.debug_tensor(t, 1)
                diff = _bits(alone[0]) != _bits(full[2])
                assert not diff.any(), f"{what} tensor {t}: frame 2 alone differs from frame 2 of the batch in {int(diff.sum())} of {diff.size} elements"
        eng.close()
    if case.dtype == "i8":
        # _fp16_gate's 99.9 % bit-identical share, over the elements of all six sizes: a 3 x 128 x 1 x 1 tensor alone has fewer than 1000
        assert total >= 3 * sum(h * w for h, w in TINY) * 32 and same >= 0.999 * total, f"{name}: only {same} of {total} elements bit-identical"


# ---------------------------------------------------------------- output transforms on head maps of 1 x 1, 1 x 3 and 2 x 3
@pytest.mark.parametrize("dtype", ["f16", "f32"])
@guarded
def test_output_transforms_on_tiny_maps(hp, monkeypatch, dtype):
    """test_engine_gpu.py::test_output_transforms' graph and outputs - pixel shuffle x 2 + group 5 + sigmoid / softplus masks + crop, and
    grid 1 / 2 with a scale - with the crop taken down to 2 fh - 1 x 2 fw - 1: 1 x 1 from a head map of one pixel."""
    _set_env(monkeypatch, {})
    for h, w in ((2, 2), (1, 5), (3, 5)):
        fh, fw = (h + 1) // 2, (w + 1) // 2
        net = Net(11)
        a = net.conv(0, 3, 32, 3, 2)
        t = net.conv(a, 32, 40, 1, act=E.ACT_NONE)  # 40 = 2 groups x 5 comps x 4 sub-pixels
        fr = _frames(2, h, w, seed=3)
        outs = [Out("a_shuf", t, 0, 40, shuffle=2, group=5, sigmoid_mask=1, softplus_mask=1 << 4, out_h=2 * fh - 1, out_w=2 * fw - 1),
                Out("b_gridx", t, 0, 16, act=E.ACT_SIGMOID, scale=32.0, grid=1),
                Out("c_gridy", t, 16, 8, act=E.ACT_SIGMOID, scale=8.0, grid=2),
                Out("d_scaled", t, 24, 16, act=E.ACT_SIGMOID, scale=384.0)]
        eng = E.Engine(net.layers, [o.c() for o in outs], net.blob(), w, h, 2, dtype=dtype)
        got = eng.inference(fr)
        assert [s for _, s, _ in eng.outputs] == [(10, 2 * fh - 1, 2 * fw - 1), (16, fh, fw), (8, fh, fw), (16, fh, fw)]
        ref = ref_net.run(net.layers, outs, net.blob(), frames_u8=fr, match_fp16=dtype == "f16")
        _check(got, ref, 2, rel=2e-3, abs_=2e-3)
        footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), 2, f"transforms {dtype} {h}x{w}")
        eng.close()


# ---------------------------------------------------------------- the built-in topologies at their smallest input
SMALLEST = [(32, 32), (35, 33)]       # (h, w): deepest maps 1 x 1 and 2 x 2 behind ResNet-50's stride 32, 4 x 4 and 5 x 5 behind the stride-8 backbones


@functools.lru_cache(maxsize=None)
def _model_reference(arch, h, w, match_fp16):
    m = E.Model(arch, w, h)
    fr = _frames(2, h, w, seed=8)
    return ref_net.run(m.layers, m.outputs, m.init_weights(3), frames_u8=fr, match_fp16=match_fp16, mean=m.mean, inv_std=m.inv_std)


@pytest.mark.parametrize("dtype", ["f16", "f32", "f32s", "i8"])
@pytest.mark.parametrize("arch", ARCHS)
@guarded
def test_builtin_topologies_at_the_smallest_input(hp, monkeypatch, arch, dtype):
    _set_env(monkeypatch, {})
    for h, w in SMALLEST:
        what = f"{arch} {dtype} {h}x{w}"
        m = E.Model(arch, w, h)
        eng = E.Engine.from_model(m, m.init_weights(3), max_batch=3, dtype=dtype)
        fr = _frames(2, h, w, seed=8)
        if dtype == "i8":
            eng.calibrate(_frames(4, h, w, seed=99))
        ids = footprint.tensor_ids(m.layers)
        both = eng.inference(fr)
        assert footprint.assert_zero_outside(eng, ids, 2, what) >= 3
        if dtype == "i8":   # (the accuracy metric of the int8 engines: test_engine_int8_gpu.py)
            assert all(np.isfinite(arr).all() for per in both for _, arr in per), what
        else:
            ref = _model_reference(arch, h, w, dtype == "f16")
            assert [nm for nm, _ in both[0]] == sorted(ref)
            for b in range(2):
                for nm, arr in both[b]:
                    if dtype == "f16":
                        _close(arr, ref[nm][b], rel=2e-2, abs_=5e-3)
                    else:
                        _close32(arr, ref[nm][b], f"{what} {nm}")
            if dtype != "f16":
                assert eng.split_fallbacks == 0
        for b in (1, 0):    # a frame alone equals the same frame of the batch, bit for bit
            one = eng.inference(fr[b:b + 1])
            for (nm, x), (_, y) in zip(one[0], both[b]):
                assert np.array_equal(_bits(x), _bits(y)), (what, nm, b)
            footprint.assert_zero_outside(eng, ids, 1, what + " n=1")
        eng.close()
