"""GPU: the "rows" form of the fp32 Winograd kernel (conv32_winograd.hip): tile rows numbered per image - ceil(H / 2) of them each - so that
the grid holds only the tile rows that exist; in a block that holds an image boundary the tile rows below it take the upper image's bottom halo
row for their own top halo row and go on with the lower image's rows.  Same tiles of every image, same arithmetic: every output byte equals the per-image
form's (HP_WINO_TALL=0).  The shapes are the smallest at which the numbering can go wrong: at least 8 tile rows per image, a batch of three or
more, boundaries at different offsets inside the blocks, even and odd H, a ragged last column of tiles.
"""
import numpy as np
import pytest

from hyperpose_amd import engine as E
from hyperpose_amd import synth
from test_engine_fp32_gpu import _run32
from test_engine_gpu import Net, Out, _frames

pytestmark = pytest.mark.gpu


def _same(got, ref, what):
    for (nm, x), (nm2, y) in zip(got, ref):
        assert nm == nm2 and np.array_equal(x, y), (nm, what)


# 160 x 144: an 18 x 20 map (9 tile rows per image), 168 x 136: a 17 x 21 map (odd H: the fourth patch row of the last tile row lies beyond the
# halo); pifpaf at 97 x 97: a 25-row map (13 tile rows: rows form) and a 13-row one (7 tile rows: the tall form with separator rows)
@pytest.mark.parametrize("arch,w_,h_,n", [("lw_openpose_mobilenet", 160, 144, 5), ("lw_openpose_mobilenet", 168, 136, 5), ("pifpaf_resnet50", 97, 97, 4)])
def test_winograd_rows_form_is_bit_identical(hp, arch, w_, h_, n, monkeypatch):
    """Every output byte equals the per-image form's - with 16 x 8 and 8 x 8 pixel blocks (HP_WINO_NC=2 | 1), one batch or two half-batches in
    flight, captured in a graph or launched directly - and a frame alone equals the frame in a batch: the first, a middle and the last one."""
    m = E.Model(arch, w_, h_)
    w = m.init_weights(5)
    fr = synth.images_u8(synth.rng_for(55), n, h_, w_)
    monkeypatch.setenv("HP_WINO_TALL", "0")
    ref_eng = E.Engine.from_model(m, w, max_batch=n, dtype="f32")
    ref_eng.set_graph(False)
    ref = ref_eng.inference(fr)
    monkeypatch.delenv("HP_WINO_TALL")
    for nc in ("1", "2"):
        monkeypatch.setenv("HP_WINO_NC", nc)
        eng = E.Engine.from_model(m, w, max_batch=n, dtype="f32")
        for graph in (True, False):
            eng.set_graph(graph)
            for conc in (1, 2):
                eng.set_concurrency(conc)
                got = eng.inference(fr)
                for b in range(n):
                    _same(got[b], ref[b], (b, nc, graph, conc))
        eng.set_concurrency(1)
        for b in (0, n // 2, n - 1):
            _same(eng.inference(fr[b:b + 1])[0], ref[b], (b, nc, "alone"))


@pytest.mark.parametrize("res_before_act", [0, 1])
def test_winograd_rows_single_layer_with_residual(hp, res_before_act, monkeypatch):
    """One 32 -> 64 layer on a 17 x 11 map, batch 3 (9 tile rows per image: 27 tile rows in four blocks, a boundary in two of them), PReLU slopes
    and a residual before / after the activation - the residual quads are requested ahead of the output transform: against the oracle at the
    engine's tolerance, against the direct kernel (HP_NO_WINOGRAD32=1) at 2e-5 of scale, and bit for bit against the per-image form."""
    h, w = 17, 11

    def build():
        net = Net(77)
        t0 = net.conv(0, 3, 32, 3, 1)
        r = net.conv(t0, 32, 64, 1, 1, act=E.ACT_NONE)
        y = net.conv(t0, 32, 64, 3, 1, res=r, res_before_act=res_before_act, act=E.ACT_PRELU)
        z = net.conv(y, 64, 24, 1, 1, act=E.ACT_NONE)  # (a network output keeps the direct kernel for its NCHW copy)
        return net, [Out("z", z, 0, 24)]
    frames = _frames(3, h, w, seed=17)
    net, outs = build()
    eng, got, _ = _run32(net, outs, frames, h, w, dtype="f32")
    assert sum(p["tile"] // 1000 == 35003 for p in eng.profile(3, iters=1)) == 1
    for b in (0, 1, 2):
        _same(eng.inference(frames[b:b + 1])[0], got[b], (b, "alone"))
    monkeypatch.setenv("HP_WINO_TALL", "0")
    net1, outs1 = build()
    _, got1, _ = _run32(net1, outs1, frames, h, w, dtype="f32")
    for b in range(3):
        _same(got[b], got1[b], (b, "per image"))
    monkeypatch.delenv("HP_WINO_TALL")
    monkeypatch.setenv("HP_NO_WINOGRAD32", "1")
    net2, outs2 = build()
    eng2, got2, _ = _run32(net2, outs2, frames, h, w, dtype="f32")
    assert not [p for p in eng2.profile(3, iters=1) if p["tile"] // 1000 == 35003]
    for b in range(3):
        for (nm, x), (_, yv) in zip(got[b], got2[b]):
            assert np.abs(x - yv).max() <= 2e-5 * np.abs(yv).max() + 1e-6, nm
