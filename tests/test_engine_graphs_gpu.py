"""GPU: the engine's fusion passes (csrc/engine.cpp: mark_pair_fusions, fuse_chains, fuse_bottlenecks, fuse_sep_pairs, pair_heads and the
fused fp32 output copy of bind_outputs) on graphs that step OFF the canonical pattern.

The kernel tests (test_engine_gpu.py, test_engine_fp32_gpu.py) run every fused kernel on the pattern the built-in models produce.  Here every
family's canonical graph is perturbed one way at a time - another reader of the tensor a fusion would elide, a concat slice in front of or
behind the pattern, another activation, another residual placement, another geometry, the pattern's result exported once, twice or in part,
the smallest maps, a foreign layer inside the pattern - and every case asserts

  * oracle: outputs against oracle/ref_net.py at the tolerance of the family's kernel test;
  * every live tensor: hp_engine_debug_tensor of every tensor of the graph equals the oracle's, or raises and nothing outside the fused
    launch needs it ("elided but still needed" is the silent failure of a wrong yes);
  * per-layer schedule: a second engine with the family's switch off, at the family's cross-schedule tolerance, bit for bit where the two
    engines run the same launches;
  * fired or refused: each row says which fused launches the engine must report (hp_engine_profile), derived from the pass's conditions;
  * batch invariance: the last frame alone gives the bits it gives inside the batch.

A CPU twin evaluates every case with the oracle alone (finite, non-constant outputs of the expected shapes) and keeps the tables honest:
per family the canonical case and at least three perturbed cases fire, at least three are refused.

How "refused" is counted: a row is refused when the per-layer schedule runs ([]), or - where the family IS an option on top of launches
that fuse anyway (PARTIAL_IS_REFUSAL: the pairing of two heads) - when that option is not taken.
"""
import zlib

import numpy as np
import pytest

import footprint
from hyperpose_amd import _lib
from hyperpose_amd import engine as E
from oracle import ref_net
from test_engine_fp32_gpu import _close32
from test_engine_gpu import Net, Out, _check, _close, _frames

CONV, DW = E.OP_CONV, E.OP_DWCONV
NONE, RELU, RELU6, LEAKY, PRELU = E.ACT_NONE, E.ACT_RELU, E.ACT_RELU6, E.ACT_LEAKY, E.ACT_PRELU


class Ref:
    """Channels [coff, coff + c) of tensor t; `layer`: the pattern layer that wrote them."""

    def __init__(self, t, coff, c, layer=None):
        self.t, self.coff, self.c, self.layer = t, coff, c, layer


def _out_hw(hw, k, stride, dil, pads):
    if pads is not None:
        return ((hw[0] + pads[0] + pads[2] - ((k - 1) * dil + 1)) // stride + 1, (hw[1] + pads[1] + pads[3] - ((k - 1) * dil + 1)) // stride + 1)
    return (-(-hw[0] // stride), -(-hw[1] // stride))


class G:
    """One case: a family's graph with the perturbation P = (kind, args...) applied while it is built.

    Tensors a perturbation needs next to the pattern (an unrelated residual, the other writer of a concat buffer) are written BEFORE the
    pattern's first layer - a layer between two pattern layers is a perturbation of its own ("between") - so a case is built twice: the first
    pass finds out which are wanted (`want`), the second creates them behind the stem."""

    def __init__(self, seed, frame_hw, P, given=None):
        self.net, self.P = Net(seed), P or (None,)
        self.h, self.w = frame_hw
        self.hw, self.outs, self.inside, self.refs = {0: frame_hw}, [], set(), {}
        self.want, self.given, self.have, self.safe = [], given, {}, None
        self.n = 2 if self.P[0] == "batch" else 3
        self.max_batch = 3
        self.seg, self.seg_of, self.kinds = 0, {}, []     # compositions: the segment every pattern layer belongs to, the segments' families

    # ---- layers
    def add(self, src, cout, k=1, stride=1, dil=1, pads=None, cin=None, in_coff=None, **kw):
        t_in, coff, c = (0, 0, 3) if src is None else (src.t, src.coff, src.c)
        t = self.net.conv(t_in, c if cin is None else cin, cout, k, stride, dil, in_coff=coff if in_coff is None else in_coff, **kw)
        L = self.net.layers[-1]
        if pads is not None:
            L.pad_explicit = 1
            L.pad[:] = list(pads)
        self.hw[t] = _out_hw(self.hw[t_in], k, stride, dil, pads)
        return Ref(t, kw.get("out_coff", 0), cout)

    def aux(self, key, hw, cout, out_coff=0):
        """A tensor of size hw the pattern does not produce (channels [out_coff, +cout) of a new tensor), from the stem's output."""
        key = (self.seg, key)
        if self.given is not None:
            return self.have[key]
        self.want.append((key, hw, cout, out_coff))
        return self._make_aux(hw, cout, out_coff)

    def _make_aux(self, hw, cout, out_coff):
        src, t = self.safe, self.net.new_tensor()
        for stride in (1, 2, 4):
            if _out_hw(self.hw[src.t], 1, stride, 1, None) == hw:
                return self.add(src, cout, 1, stride, act=LEAKY, act_param=0.1, out=t, out_coff=out_coff)
        assert _out_hw(self.hw[src.t], 1, 1, 1, (1, 1, 1, 1)) == hw, (self.hw[src.t], hw)
        return self.add(src, cout, 1, pads=(1, 1, 1, 1), act=LEAKY, act_param=0.1, out=t, out_coff=out_coff)

    def stem_done(self, safe):
        self.safe = safe
        for key, hw, cout, out_coff in (self.given or []):
            self.have[key] = self._make_aux(hw, cout, out_coff)

    def stem_conv(self, src, cout, k, stride, sliced=False, act=RELU):
        """A stem convolution; `sliced`: under the "in_coff" perturbation its output is channels [off, off + cout) of a concat buffer."""
        if sliced and self.P[0] == "in_coff":
            off, cat = self.P[1], self.net.new_tensor()
            self.add(src, off, k, stride, act=LEAKY, act_param=0.1, out=cat, out_coff=0)
            return self.add(src, cout, k, stride, act=act, out=cat, out_coff=off)
        return self.add(src, cout, k, stride, act=act)

    def layer(self, i, src, cout, k=1, stride=1, dil=1, op=CONV, act=RELU, act_param=0.0, res=None, rba=0, last=False, into=None):
        """Pattern layer i, with whatever the perturbation says about it."""
        P, kind = self.P, self.P[0]
        if kind == "between" and P[1] == i:   # an unrelated layer in the layer list right in front of pattern layer i
            u = self.add(None, 8, 3, 1)
            self.outs.append(Out("u", u.t, 0, 8))
        pads = None
        if kind == "act" and P[1] == i:
            act, act_param = P[2], (P[3] if len(P) > 3 else 0.0)
        if kind == "geom" and P[1] == i:
            stride = {"stride2": 2, "stride1": 1}.get(P[2], stride)
            dil = 2 if P[2] == "dil2" else dil
            pads = (1, 0, 1, 2) if P[2] == "pads" else (1, 1, 1, 1) if P[2] == "pad1x1" else None
        if kind == "other_in" and P[1] == i:      # this layer reads another tensor of the same shape
            src = self.aux("in", self.hw[src.t], src.c)
        cin, in_coff = src.c, src.coff
        if kind == "sub" and src.layer == P[1]:
            cin, in_coff = src.c - 32, src.coff + 8
            cout = cin if op == DW else cout
        ohw = _out_hw(self.hw[src.t], k, stride, dil, pads)
        if kind == "res" and P[1] == i:
            if P[2] == "flip":
                rba = 1 - rba
            elif P[2] == "none":
                res = None
            elif P[2] == "x":
                res = self.refs["x"]
            elif P[2] == "mid":
                res = self.refs[P[3]]
            elif P[2] == "other":
                res = self.aux("res", ohw, cout)
            if len(P) > 4:
                rba = P[4]
        assert res is None or (res.coff == 0 and res.c >= cout), "a residual is channels [0, cout) of its tensor"
        out, out_coff = None, 0
        if into is not None:
            out, out_coff = into
        if kind == "mid_concat" and P[1] == i:   # the layer's output is the front of a concat buffer another layer writes as well
            out = self.aux("cat", ohw, 8, out_coff=cout).t
        if kind == "out_coff" and last:          # ... or a slice behind another writer's channels, read as a whole further down
            out, out_coff = self.aux("front", ohw, P[1]).t, P[1]
        kw = dict(out=out) if out is not None else {}
        r = self.add(src, cout, k, stride, dil, pads, cin=cin, in_coff=in_coff, op=op, act=act, act_param=act_param, out_coff=out_coff,
                     res=res.t if res is not None else -1, res_before_act=rba, **kw)
        r.layer = i
        self.inside.add(len(self.net.layers) - 1)
        self.seg_of[len(self.net.layers) - 1] = self.seg
        self.refs[i] = r
        return r

    # ---- what reads the pattern
    def finish(self, lasts, tail=True):
        P, kind = self.P, self.P[0]
        for j, y in enumerate(lasts):
            final = j == len(lasts) - 1
            if kind == "outs" and final:
                if P[1] == "plain":
                    self.outs.append(Out("y", y.t, y.coff, y.c))
                elif P[1] == "twice":
                    self.outs += [Out("y1", y.t, y.coff, y.c), Out("y2", y.t, y.coff, y.c)]
                else:
                    self.outs.append(Out("ys", y.t, y.coff + 8, 8))
            if not tail:
                continue
            whole = Ref(y.t, 0, y.coff + y.c) if (kind == "out_coff" and y.coff) else y
            z = self.add(whole, 32, 1, act=NONE)
            self.outs.append(Out(f"z{j}", z.t, 0, 32))
        if kind == "reader":        # a later 1x1 also reads the would-be-elided tensor
            m = self.refs[P[1]]
            self.outs.append(Out("r", self.add(m, 32, 1, act=NONE).t, 0, 32))
        if kind == "as_res":        # ... or adds it as its residual
            m = self.refs[P[1]]
            a = self.aux("asres", self.hw[m.t], 32)
            self.outs.append(Out("ar", self.add(a, m.c, 1, act=RELU, res=m.t).t, 0, m.c))
        if kind == "mid_out":       # ... or it is a network output (P[2]: its scale)
            m = self.refs[P[1]]
            self.outs.append(Out("m", m.t, m.coff, m.c, scale=P[2]))

    def expected_shapes(self):
        return {o.name.decode(): (self.n, o.channels) + self.hw[o.tensor] for o in self.outs}


# ---------------------------------------------------------------- families
class Family:
    """stem(g) -> the tensors the pattern reads; pattern(g, x) -> the pattern's last tensors; sig(profile) -> which fused launches ran."""

    def __init__(self, name, stem, pattern, sig, map_hw, down=1, dtype="f16", env=None, off=None, tol=None, xtol=None, xbits=False, seed=0,
                 tail=True, ab=None):
        self.name, self.stem, self.pattern, self.sig, self.map_hw, self.down, self.dtype = name, stem, pattern, sig, map_hw, down, dtype
        self.env, self.off = env or {}, off or {"HP_NO_FUSE": "1"}
        self.tol, self.xtol, self.xbits, self.seed, self.tail = tol or {}, xtol or {}, xbits, seed or zlib.crc32(name.encode()) % 1000, tail
        self.ab = ab     # a switch that only changes HOW the family's launches are issued (two heads in one grid): same bits with and without


def build(fam, P, given=None):
    mh, mw = (P[1], P[2]) if P and P[0] == "size" else fam.map_hw
    g = G(fam.seed, (mh * fam.down, mw * fam.down), P, given)
    x = fam.stem(g)
    lasts = fam.pattern(g, x)
    g.finish(lasts, fam.tail)
    if given is None and g.want:
        return build(fam, P, g.want)
    return g


def _plain_stem(c, down=1, sliced=True):
    def stem(g):
        t = None
        if down == 4:
            t = g.add(None, 32, 3, 2)
            x = g.stem_conv(t, c, 3, 2, sliced)
        else:
            x = g.stem_conv(t, c, 3, 1, sliced)
        g.refs["x"] = x
        g.stem_done(x)
        return x
    return stem


def _ops(prof, op, base):
    return [p["tile"] - base for p in prof if p["op"] == op]


def sig_sep(prof):       # sepconv launches that are not the pair kernel: their variant
    return [v for v in _ops(prof, 100, 4000000) if v != 20]


def sig_seppair(prof):
    return [v for v in _ops(prof, 100, 4000000) if v == 20]


def sig_head(prof):      # fused two-layer heads: one entry per launch
    return _ops(prof, 101, 6000000)


def sig_chain(prof):
    return _ops(prof, 102, 7000000)


def sig_bneck(prof):
    return _ops(prof, 103, 9000000)


def sig_sep32(prof):     # conv32_direct_kernel's depthwise-fused forms
    return [1 for p in prof if p["tile"] >= 33000000 and p["tile"] // 100000 % 10 in (1, 2) and p["tile"] // 1000000 in (33, 34)]


def sig_head32(prof):
    return [1 for p in prof if p["tile"] // 1000000 == 37]


def pat_sep(c, cout, stride=1, dil=1):
    def f(g, x):
        d = g.layer(0, x, c, 3, stride, dil, op=DW, act=RELU6)
        return [g.layer(1, d, cout, 1, act=RELU, last=True)]
    return f


def pat_seppair(g, x):
    d1 = g.layer(0, x, 32, 3, op=DW, act=RELU6)
    p1 = g.layer(1, d1, 64, 1, act=RELU6)
    d2 = g.layer(2, p1, 64, 3, 2, op=DW, act=RELU6)
    return [g.layer(3, d2, 128, 1, act=RELU6, last=True)]


def pat_head(g, x):
    a = g.layer(0, x, 512, 1, act=RELU)
    return [g.layer(1, a, 19, 1, act=NONE, last=True)]


def pat_headpair(g, x):
    a = g.layer(0, x, 512, 1, act=RELU)
    y1 = g.layer(1, a, 19, 1, act=NONE)
    b = g.layer(2, x, 512, 1, act=RELU)
    return [y1, g.layer(3, b, 38, 1, act=NONE, last=True)]


def sig_headpair(prof):
    """[2]: ONE launch for both heads (its row stands for four consecutive layers, none of which has a row of its own);
    otherwise one 1 per single-head launch."""
    rows = [p["layer"] for p in prof if p["op"] == 101]
    if len(rows) == 1 and not any(rows[0] < p["layer"] <= rows[0] + 3 for p in prof):
        return [2]
    return [1] * len(rows)


def pat_chain2(g, x):
    v = g.layer(0, x, 128, 3)
    return [g.layer(1, v, 128, 3, last=True)]


def pat_chain3(g, x):
    u = g.layer(0, x, 128, 1)
    v = g.layer(1, u, 128, 3)
    return [g.layer(2, v, 128, 3, res=u, last=True)]


def _bneck_stem(g):      # block input x (256 channels, the shortcut) and the block's own reduction r: a launch of its own, the pattern's input
    t = g.add(None, 32, 3, 2)
    x = g.add(t, 256, 3, 2)
    g.refs["x"] = x
    g.stem_done(x)
    return g.stem_conv(x, 64, 1, 1, sliced=True)


def pat_bneck_front(g, r):
    v = g.layer(0, r, 64, 3)
    return [g.layer(1, v, 256, 1, res=g.refs["x"], rba=1, last=True)]


def pat_bneck_next(g, r):
    v = g.layer(0, r, 64, 3)
    y = g.layer(1, v, 256, 1, res=g.refs["x"], rba=1)
    return [y, g.layer(2, y, 64, 1, last=True)]


def pat_bneck_proj(g, x):
    pj = g.layer(0, x, 256, 1, act=NONE)
    r = g.layer(1, x, 64, 1)
    v = g.layer(2, r, 64, 3)
    return [g.layer(3, v, 256, 1, res=pj, rba=1, last=True)]


def _stage32_stem(g):    # LW-OpenPose's stage layout: a concat buffer [128 trunk features | 19 heat-maps | 38 PAFs], the heads read a 1x1 of its front
    t0 = g.add(None, 32, 3, 1)
    cat = g.net.new_tensor()
    g.add(t0, 128, 3, 1, out=cat, out_coff=0)
    g.refs["cat"] = Ref(cat, 0, 185)
    trunk = g.stem_conv(Ref(cat, 0, 128), 128, 1, 1, sliced=True)
    g.refs["x"] = trunk
    g.stem_done(trunk)
    return trunk


def pat_stage32(g, x):
    cat = g.refs["cat"].t
    a = g.layer(0, x, 512, 1, act=RELU)
    g.layer(1, a, 19, 1, act=NONE, into=(cat, 128))
    b = g.layer(2, x, 512, 1, act=RELU)
    g.layer(3, b, 38, 1, act=NONE, into=(cat, 147))
    nxt = g.add(g.refs["cat"], 128, 1)
    y = g.add(nxt, 24, 3, act=NONE)
    g.outs += [Out("conf", cat, 128, 19), Out("paf", cat, 147, 38), Out("y", y.t, 0, 24)]
    if g.P[0] == "outs":     # the heat-maps under a second name / a part of the PAFs
        g.outs.append(Out("conf2", cat, 128, 19) if g.P[1] == "twice" else Out("paf_part", cat, 151, 8))
    return []


# (fp32 families compare with test_engine_fp32_gpu.py's _close32, REL, ABS = 1e-4, 1e-6, and across schedules at its 2e-5 of scale + 1e-6)
X32 = dict(rel=2e-5, abs_=1e-6)
FAMILIES = {f.name: f for f in [
    Family("sep64s2", _plain_stem(64), pat_sep(64, 128, 2), sig_sep, (23, 27), xbits=True),
    Family("sep128", _plain_stem(128), pat_sep(128, 128), sig_sep, (23, 27), xbits=True),
    Family("sep32", _plain_stem(32), pat_sep(32, 64), sig_sep, (23, 27), xbits=True),
    Family("sep512", _plain_stem(512), pat_sep(512, 512), sig_sep, (23, 27), xbits=True),
    Family("seppair", _plain_stem(32), pat_seppair, sig_seppair, (23, 27), xbits=True),
    Family("head", _plain_stem(128), pat_head, sig_head, (17, 12), xtol=dict(rel=2e-3, abs_=1e-3)),
    Family("headpair", _plain_stem(128), pat_headpair, sig_headpair, (17, 12), xtol=dict(rel=2e-3, abs_=1e-3), ab={"HP_NO_PAIR_HEADS": "1"}),
    Family("chain2", _plain_stem(128, 4), pat_chain2, sig_chain, (13, 17), down=4, xtol=dict(rel=2e-3, abs_=1e-3)),
    Family("chain3", _plain_stem(128, 4), pat_chain3, sig_chain, (13, 17), down=4, xtol=dict(rel=2e-3, abs_=1e-3)),
    Family("bneck_front", _bneck_stem, pat_bneck_front, sig_bneck, (13, 19), down=4, tol=dict(rel=3e-3), xtol=dict(rel=4e-3, abs_=2e-3)),
    Family("bneck_next", _bneck_stem, pat_bneck_next, sig_bneck, (13, 19), down=4, tol=dict(rel=3e-3), xtol=dict(rel=4e-3, abs_=2e-3)),
    Family("bneck_proj", _plain_stem(64, 4), pat_bneck_proj, sig_bneck, (13, 19), down=4, tol=dict(rel=4e-3, abs_=2e-3),
           xtol=dict(rel=4e-3, abs_=4e-3)),
    Family("sep32_f32s", _plain_stem(64), pat_sep(64, 128), sig_sep32, (23, 27), dtype="f32s", off={"HP_NO_FUSE32": "1"}, xtol=X32),
    Family("sep32_f32", _plain_stem(64), pat_sep(64, 128), sig_sep32, (23, 27), dtype="f32", env={"HP_FUSE32": "1"},
           off={"HP_FUSE32": "1", "HP_NO_FUSE32": "1"}, xtol=X32),
    Family("head32", _plain_stem(128), pat_head, sig_head32, (17, 12), dtype="f32", off={"HP_NO_HEAD32": "1"}, xtol=X32),
    Family("stage32", _stage32_stem, pat_stage32, sig_head32, (17, 12), dtype="f32", off={"HP_NO_HEAD32": "1"}, xtol=X32, tail=False, ab={"HP_HEAD_PAIR": "0"}),
]}

# ---------------------------------------------------------------- the perturbation matrix
# Rows: (perturbation, the fused launches the engine must report, why).  The expectation is read off the pass's conditions; where the
# kernel family's own `variant` function decides, the row names it.  [] = refused: the per-layer schedule runs.
A0, A1 = 0.1, 0.0


# families that are an option on top of launches which fuse anyway: a row where the option is not taken (two single-head launches instead of
# the pair; one of the stage's two heads left to the per-layer kernels) is that family's refusal
PARTIAL_IS_REFUSAL = {"headpair", "stage32"}


def _pid(P):
    return "canonical" if P is None else "-".join(str(a) for a in P)

SIZES = [("size", 1, 1), ("size", 1, 9), ("size", 9, 1)]


def _sep_rows(v, c, cout, stride, full=False):
    """mark_pair_fusions, fuse_kind::sep: the depthwise layer's tensor has ONE reader (the next layer, a plain unpadded 1x1 without residual
    that reads all of it from channel 0), ONE writer, is no output; relu / relu6 on the depthwise half; TF-SAME geometry; the block's
    result is no network output; sepconv_variant_for(C, Cout, stride, dilation) has an instance."""
    rows = [(None, [v], "canonical"), (("batch",), [v], "n < max_batch"), (("size", 9, 7), [v], "smaller than one tile")] + [(s, [v], "tiny map") for s in SIZES]
    rows += [(("reader", 0), [], "second reader"), (("as_res", 0), [], "read as a residual"), (("mid_out", 0, 0.0), [], "network output"),
             (("mid_out", 0, 2.0), [], "scaled network output"), (("mid_concat", 0), [], "tensor C != cout")]
    if c > 32:
        rows.append((("sub", 0), [], "Bn.in_coff != 0 / Bn.cin != A.cout"))
    rows += [(("in_coff", 8), [v], "A.in_coff % 8 == 0"), (("in_coff", 32), [v], ""), (("out_coff", 8), [v], "Bn.out_coff % 8 == 0"), (("out_coff", 32), [v], "")]
    rows += [(("act", 0, NONE), [], "depthwise act must be relu / relu6"), (("act", 0, LEAKY, A0), [], ""), (("act", 0, LEAKY, A1), [], "act != RELU although it computes relu"),
             (("act", 0, RELU), [v], "")]
    rows += [(("act", 1, a, p), [v], "any pointwise activation but sigmoid / softplus") for a, p in ((NONE, 0), (LEAKY, A0), (LEAKY, A1), (PRELU, 0), (RELU6, 0))]
    rows += [(("res", 1, "other"), [], "Bn.res >= 0")]
    if c == cout and stride == 1:
        rows += [(("res", 1, "x"), [], "Bn.res >= 0"), (("res", 1, "mid", 0), [], "Bn.res >= 0")]
    other = {(64, 2): ("stride1", [1]), (128, 1): ("stride2", [2]), (32, 1): ("stride2", []), (512, 1): ("stride2", [])}[(c, stride)]
    rows += [(("geom", 0, other[0]), other[1], "sepconv_variant_for at the other stride"),
             (("geom", 0, "pads"), [], "explicit pads differ from TF-SAME"), (("geom", 1, "pad1x1"), [], "the 1x1 half must not pad")]
    if stride == 1:     # (stride 2 with dilation 2 has no depthwise kernel at all: test_depthwise_without_a_kernel_is_refused_when_built)
        rows += [(("geom", 0, "dil2"), [6] if c == 512 else [], "sepconv_variant_for: dilation 2 only in the 512-output form")]
    rows += [(("outs", k), [], "the block's result is a network output: generic epilogue") for k in ("plain", "twice", "sub")]
    rows += [(("between", 1), [], "Bn is layers[i + 1]")]
    if not full:    # the other instances of the kernel: what depends on the instance (sizes, slices, geometry, the epilogue's forms)
        keep = ("canonical", "batch", "size", "in_coff", "out_coff", "geom", "reader", "mid_concat", "sub")
        rows = [r for r in rows if _pid(r[0]).split("-")[0] in keep or r[0][:3] in (("act", 1, PRELU), ("act", 1, NONE), ("act", 0, NONE))]
    return rows


def _seppair_rows():
    """fuse_sep_pairs: two consecutive OP_SEPCONV steps, the tensor between them private (one reader, one writer, no output),
    seppair_variant: 32 -> 64 stride 1 then 64 -> 128 stride 2, relu-family clamp on the first block's 1x1, no fp32 copy."""
    v = [20]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 9, 7), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 1), [], "not private"), (("reader", 0), [], "block a is not fused"), (("as_res", 1), [], ""), (("mid_out", 1, 0.0), [], "block a's result is an output: not a sepconv step"),
             (("mid_out", 1, 2.0), [], ""), (("mid_concat", 1), [], "writers != 1"),
             (("sub", 1), [], "Db.in_coff != Pa.out_coff (and a 32-channel stride-2 block has no fused instance)")]
    rows += [(("in_coff", 8), v, ""), (("in_coff", 32), v, ""), (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    rows += [(("act", 1, NONE), [], "qa.act_slope != 0"), (("act", 1, LEAKY, A0), [], ""), (("act", 1, LEAKY, A1), v, "slope 0 is a relu clamp"), (("act", 1, PRELU), [], "qa.alpha"),
             (("act", 1, RELU), v, ""), (("act", 3, NONE), v, "block b's epilogue is the generic fast one"), (("act", 3, LEAKY, A0), v, ""), (("act", 3, PRELU), v, ""),
             (("act", 0, NONE), [], "block a not fused"), (("act", 2, LEAKY, A0), [], "block b not fused"), (("act", 2, RELU), v, "")]
    rows += [(("res", 3, "other"), [], "block b not fused"), (("res", 1, "other"), [], "block a not fused")]
    rows += [(("geom", 0, "stride2"), [], "a.stride != 1"), (("geom", 2, "stride1"), [], "b.stride != 2"), (("geom", 0, "dil2"), [], ""), (("geom", 2, "pads"), [], ""),
             (("geom", 1, "pad1x1"), [], "")]
    rows += [(("outs", k), [], "block b's result is an output") for k in ("plain", "twice", "sub")]
    rows += [(("between", 2), [], "the two sepconv steps are not consecutive"), (("between", 1), [], "")]
    return rows


def _head_rows(v, f32=False):
    """mark_pair_fusions, fuse_kind::head / head32: 1x1 K1 -> 512 (relu / relu6; head32: none / relu / relu6 / leaky) whose tensor has one reader - the next
    layer, an unpadded 1x1 to <= 64 channels without residual - one writer and is no output.  The second layer may write a slice and may be
    a network output (the kernel writes the fp32 copy)."""
    o1, o2 = (4, 4) if f32 else (8, 32)
    rows = [(None, v, "canonical"), (("batch",), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [], ""), (("as_res", 0), [], ""), (("mid_out", 0, 0.0), [], ""), (("mid_out", 0, 2.0), [], ""), (("mid_concat", 0), [], "tensor C != cout"),
             (("sub", 0), [], "Bn.in_coff != 0")]
    rows += [(("in_coff", o1), v, "")] + ([] if f32 else [(("in_coff", o2), v, "")])
    rows += [(("out_coff", 147), v, "")] if f32 else [(("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    wide = v if f32 else []
    rows += [(("act", 0, NONE), wide, "hidden activation"), (("act", 0, LEAKY, A0), wide, ""), (("act", 0, LEAKY, A1), wide, "fp16: act != RELU although it computes relu"),
             (("act", 0, PRELU), [], "per-channel slopes on the hidden layer"), (("act", 0, RELU6), v, "")]
    rows += [(("act", 1, a, p), v, "") for a, p in ((RELU, 0), (LEAKY, A0), (LEAKY, A1), (PRELU, 0), (RELU6, 0))]
    rows += [(("res", 1, "other"), [], "Bn.res >= 0"), (("res", 0, "other"), [], "A.res >= 0")]
    rows += [(("geom", 0, "stride2"), [], ""), (("geom", 0, "pad1x1"), [], "padded 1x1"), (("geom", 1, "pad1x1"), [], "")]
    rows += [(("outs", k), v, "the kernel writes the fp32 copy / the conversion kernel reads the fp16 slice") for k in ("plain", "twice", "sub")]
    rows += [(("between", 1), [], "")]
    return rows


def _headpair_rows():
    """pair_heads: two consecutive OP_MLPHEAD steps with the same input view, K1 and map."""
    v = [2]
    rows = [(None, v, "canonical"), (("batch",), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("in_coff", 8), v, ""), (("in_coff", 32), v, ""), (("out_coff", 8), v, ""), (("out_coff", 32), v, ""), (("act", 0, RELU6), v, "each head keeps its own clamp"),
             (("act", 1, LEAKY, A0), v, ""), (("act", 3, PRELU), v, ""), (("outs", "plain"), v, ""), (("outs", "twice"), v, ""), (("outs", "sub"), v, "")]
    rows += [(("act", 2, NONE), [1], "the second head is not fused"), (("reader", 0), [1], "the first head is not fused"), (("mid_out", 2, 0.0), [1], ""),
             (("between", 2), [1, 1], "the two head steps are not consecutive"), (("geom", 3, "pad1x1"), [1], ""), (("res", 1, "other"), [1], ""),
             (("as_res", 0), [1], "the first head's hidden tensor is read elsewhere"), (("mid_concat", 0), [1], "tensor C != cout"),
             (("other_in", 2), [1, 1], "x.in.p != y.in.p: the heads read different tensors (a rule of the pass, not of the kernel: each head of the pair kernel has its own parameter block)")]
    return rows


def _chain2_rows():
    """fuse_chains, 2-form: consecutive plain 3x3 steps, the second reads exactly what the first writes, that tensor has no other reader /
    writer and is no output, at most one residual and not the intermediate; conv_chain_variant: 128 -> 128, stride 1, dilation 1, pad 1,
    one-clamp activations (slope 0, no PReLU), residual after the activation, no fused fp32 copy."""
    v = [1]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 2, 2), v, "everything is halo")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [], ""), (("as_res", 0), [], ""), (("mid_out", 0, 0.0), [], ""), (("mid_out", 0, 2.0), [], ""), (("mid_concat", 0), [], "writers != 1"),
             (("sub", 0), [], "Cn.in_coff != Bn.out_coff")]
    rows += [(("in_coff", 8), v, ""), (("in_coff", 32), v, ""), (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    for i in (0, 1):
        rows += [(("act", i, NONE), [], "act_slope != 0"), (("act", i, LEAKY, A0), [], ""), (("act", i, LEAKY, A1), v, "slope 0"), (("act", i, PRELU), [], "alpha"), (("act", i, RELU6), v, "")]
    rows += [(("res", 0, "x"), [2], "res_mode 1"), (("res", 1, "x"), [3], "res_mode 2"), (("res", 1, "other"), [3], "any tensor may be the residual"),
             (("res", 1, "mid", 0), [], "Cn.res == Bn.out"), (("res", 1, "x", None, 1), [], "res_before_act")]
    rows += [(("geom", 0, "stride2"), [], ""), (("geom", 1, "dil2"), [], ""), (("geom", 0, "pads"), [], "pad_l != 1"), (("geom", 1, "pads"), [], "")]
    rows += [(("outs", "plain"), [], "out_f32"), (("outs", "twice"), [], "the first name takes the fused copy"), (("outs", "sub"), v, "the conversion kernel reads the fp16 tensor")]
    rows += [(("between", 1), [], "steps not consecutive")]
    return rows


def _chain3_rows():
    """fuse_chains, 3-form [1x1 -> 3x3 -> 3x3 (+ the 1x1's output)]; where it is refused the two 3x3 layers may still run as the 2-form
    (variant 3: residual on the second layer), which starts at the NEXT step."""
    v = [13]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 2, 2), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [3], "the 1x1's output is read elsewhere: 2-form behind it"), (("reader", 1), [], ""), (("as_res", 0), [3], ""), (("mid_out", 0, 0.0), [3], ""),
             (("mid_out", 1, 2.0), [], ""), (("mid_concat", 0), [3], "writers != 1"), (("sub", 0), [], "c1.Cin != 128")]
    rows += [(("in_coff", 8), v, ""), (("in_coff", 32), v, ""), (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    rows += [(("act", 0, RELU6), v, ""), (("act", 0, LEAKY, A1), v, ""), (("act", 0, NONE), [3], "c0 refused by conv_chain_variant"), (("act", 0, LEAKY, A0), [3], ""),
             (("act", 0, PRELU), [3], ""), (("act", 1, NONE), [], ""), (("act", 2, NONE), [], ""), (("act", 1, RELU6), v, ""), (("act", 2, RELU6), v, "")]
    rows += [(("res", 2, "flip"), [], "res_before_act"), (("res", 2, "none"), [10], ""), (("res", 2, "other"), [3], "not the 1x1's output"), (("res", 2, "x"), [3], ""),
             (("res", 2, "mid", 1), [], "Cn.res == Bn.out")]
    rows += [(("geom", 1, "dil2"), [], ""), (("geom", 2, "pads"), [], ""), (("geom", 0, "pad1x1"), [3], "the padded 1x1 stays alone"), (("geom", 0, "stride2"), [3], "")]
    rows += [(("outs", "plain"), [], "out_f32"), (("outs", "twice"), [], ""), (("outs", "sub"), v, "")]
    rows += [(("between", 1), [3], "the 3x3 pair is still consecutive"), (("between", 2), [], "")]
    return rows


def _bneck_front_rows():
    """fuse_bottlenecks: 3x3 M -> M whose tensor only the expansion reads (one writer) + expansion 1x1 M -> 4M with any shortcut;
    bottleneck_variant: stride 1, dilation 1, pad k / 2, slope-0 activations, no fp32 copy, and a lone expansion is not taken."""
    v = [1001]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 2, 2), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [], "no 3x3 in front, no reduction: a lone expansion"), (("as_res", 0), [], ""), (("mid_out", 0, 0.0), [], ""), (("mid_out", 0, 2.0), [], ""),
             (("mid_concat", 0), [], "writers != 1"), (("sub", 0), [], "E.in_coff != A.out_coff")]
    rows += [(("in_coff", 8), v, ""), (("in_coff", 32), v, ""), (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    rows += [(("act", 0, NONE), [], "bneck_conv_ok(c3)"), (("act", 0, LEAKY, A1), v, ""), (("act", 0, RELU6), v, ""), (("act", 0, PRELU), [], ""), (("act", 1, RELU6), v, ""),
             (("act", 1, NONE), [], ""), (("act", 1, LEAKY, A0), [], "")]
    rows += [(("res", 1, "flip"), v, "the kernel honours res_before_act"), (("res", 1, "none"), v, ""), (("res", 1, "other"), v, "")]
    rows += [(("geom", 0, "dil2"), [], ""), (("geom", 0, "pads"), [], "")]
    rows += [(("outs", "plain"), [], "out_f32"), (("outs", "twice"), [], ""), (("outs", "sub"), v, "")]
    rows += [(("between", 1), [], "steps not consecutive")]
    return rows


def _bneck_next_rows():
    """... + the NEXT block's reduction 1x1 4M -> MR (relu family, stride 1, no residual, reads exactly the expansion's slice), one or two
    steps further down; what bottleneck_variant does not take is dropped and the rest still fuses."""
    v = [1011]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 2, 2), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [1010], "expansion + reduction without the 3x3"), (("mid_out", 0, 0.0), [1010], ""), (("mid_out", 0, 2.0), [1010], ""),
             (("as_res", 0), [1010], ""), (("mid_concat", 0), [1010], "writers != 1"), (("act", 1, LEAKY, A0), [], "bneck_conv_ok(ce): nothing left to fuse"),
             (("act", 1, PRELU), [], ""), (("in_coff", 8), v, ""), (("in_coff", 32), v, ""),
             (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    rows += [(("act", 2, NONE), [1001], "the reduction is dropped"), (("act", 2, LEAKY, A1), v, ""), (("act", 2, RELU6), v, ""), (("act", 2, PRELU), [1001], ""),
             (("geom", 2, "stride2"), [1001], "strided reduction"), (("sub", 1), [1001], "R.in_coff != E.out_coff"), (("res", 2, "other"), [1001], "R.res >= 0"),
             (("act", 0, NONE), [1010], "the 3x3's step starts no block (bottleneck_variant refuses c3, engine.cpp fuse_bottlenecks `if (!ok) continue`), the loop's next step, the expansion, starts one without it"),
             (("act", 1, NONE), [], "")]
    rows += [(("between", 2), v, "the reduction may sit two steps further down"), (("between", 1), [1010], "the 3x3 is not the step in front")]
    rows += [(("outs", "plain"), [1001], "the reduction writes a fused fp32 copy"), (("outs", "twice"), [1001], ""), (("outs", "sub"), v, "")]
    return rows


def _bneck_proj_rows():
    """... + the projection shortcut (1x1 64 -> 256, no activation, only this block reads it, residual before the relu) and the block's own
    reduction (1x1 of the same input slice, only the 3x3 reads it) computed inside the launch."""
    v = [1301]
    rows = [(None, v, "canonical"), (("batch",), v, ""), (("size", 2, 2), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [1001], "the projection is read elsewhere"), (("reader", 1), [1101], "the own reduction is read elsewhere"), (("reader", 2), [], "no 3x3, no reduction"),
             (("mid_out", 0, 2.0), [1001], ""), (("mid_out", 0, 0.0), [1001], ""), (("as_res", 0), [1001], "the projection is another layer's residual too"),
             (("res", 3, "none"), [1001], "no shortcut, no projection"), (("res", 3, "other"), [1001], "the shortcut's writer is no linear 1x1 of the block input"),
             (("geom", 2, "pads"), [], "bneck_conv_ok(c3)"),
             (("mid_concat", 0), [1001], "writers != 1"), (("act", 0, RELU), [1001], "P.act != NONE"), (("act", 1, NONE), [1101], "bneck_conv_ok(c0)"),
             (("act", 1, RELU6), v, ""), (("act", 2, RELU6), v, ""), (("res", 3, "flip"), [1001], "E.res_before_act"), (("in_coff", 8), v, ""), (("in_coff", 32), v, ""),
             (("out_coff", 8), v, ""), (("out_coff", 32), v, "")]
    rows += [(("between", 3), [], ""), (("between", 1), v, "the projection and the reduction are searched in front of the 3x3"), (("outs", "sub"), v, ""), (("outs", "plain"), [], "out_f32"),
             (("geom", 2, "dil2"), [], "")]
    return rows


def _sep32_rows(full=True):
    """mark_pair_fusions, fuse_kind::sep32: depthwise 3x3 stride 1, dilation 1 | 2, whole 64-channel chunks, none / relu / relu6 / leaky, TF-SAME
    geometry, one reader (the next layer, an unpadded 1x1 reading all of it) / one writer / no output; the 1x1 half may carry a residual
    (not the elided tensor), write a slice and be an output; pick32::dw_fusable has a form."""
    v = [1]
    rows = [(None, v, "canonical"), (("batch",), v, "n < max_batch"), (("size", 9, 7), v, "")] + [(s, v, "") for s in SIZES]
    rows += [(("reader", 0), [], ""), (("as_res", 0), [], ""), (("mid_out", 0, 0.0), [], ""), (("mid_out", 0, 2.0), [], ""), (("mid_concat", 0), [], ""), (("sub", 0), [], "")]
    rows += [(("in_coff", 4), v, "A.in_coff % 4 == 0"), (("out_coff", 147), v, "")]
    rows += [(("act", 0, a, p), v, "") for a, p in ((NONE, 0), (LEAKY, A0), (LEAKY, A1), (RELU, 0))]
    rows += [(("act", 1, a, p), v, "") for a, p in ((NONE, 0), (LEAKY, A0), (PRELU, 0), (RELU6, 0))]
    rows += [(("res", 1, "other"), v, "a residual on the 1x1 half is the kernel's epilogue")]
    rows += [(("geom", 0, "stride2"), [], ""), (("geom", 0, "dil2"), v, ""), (("geom", 0, "pads"), [], ""), (("geom", 1, "pad1x1"), [], "")]
    rows += [(("outs", k), v, "") for k in ("plain", "twice", "sub")]
    rows += [(("between", 1), [], "")]
    if not full:    # the same pass on the fp32 pipe (HP_FUSE32=1): the rows where the pipe's kernel form matters
        rows = [r for r in rows if _pid(r[0]).split("-")[0] in ("canonical", "batch", "size", "in_coff", "out_coff", "geom", "reader", "res", "outs", "sub", "between")]
    return rows


def _stage32_rows():
    """Two head32 launches on one input (paired at run time, pick32::head_pair_ok: not visible in the profile), writing the stage's concat
    slices at 128 and 147 which are outputs as well."""
    v = [1, 1]
    rows = [(None, v, "canonical"), (("batch",), v, "n < max_batch")] + [(s, v, "") for s in SIZES]
    rows += [(("in_coff", 4), v, ""), (("act", 0, RELU6), v, ""), (("act", 2, LEAKY, A0), v, ""), (("act", 1, PRELU), v, ""), (("outs", "twice"), v, "the heat-maps under two names"),
             (("outs", "sub"), v, ""), (("between", 2), v, "both heads still fuse")]
    rows += [(("reader", 0), [1], ""), (("mid_out", 2, 0.0), [1], ""), (("act", 0, PRELU), [1], ""), (("between", 1), [1], ""), (("res", 3, "other"), [1], "Bn.res >= 0")]
    return rows


ROWS = {
    "sep64s2": _sep_rows(2, 64, 128, 2), "sep128": _sep_rows(1, 128, 128, 1, full=True), "sep32": _sep_rows(7, 32, 64, 1), "sep512": _sep_rows(5, 512, 512, 1),
    "seppair": _seppair_rows(), "head": _head_rows([128]), "headpair": _headpair_rows(), "chain2": _chain2_rows(), "chain3": _chain3_rows(),
    "bneck_front": _bneck_front_rows(), "bneck_next": _bneck_next_rows(), "bneck_proj": _bneck_proj_rows(),
    "sep32_f32s": _sep32_rows(), "sep32_f32": _sep32_rows(full=False), "head32": _head_rows([1], f32=True), "stage32": _stage32_rows(),
}


CASES = [pytest.param(f, P, want, id=f"{f}-{_pid(P)}") for f, rows in ROWS.items() for P, want, _ in rows]


# ---------------------------------------------------------------- the checks
def _engine(monkeypatch, g, fam, env):
    for k in ("HP_NO_FUSE", "HP_FUSE32", "HP_NO_FUSE32", "HP_NO_HEAD32", "HP_NO_PAIR_HEADS", "HP_HEAD_PAIR"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = E.Engine(g.net.layers, [o.c() for o in g.outs], g.net.blob(), g.w, g.h, g.max_batch, dtype=fam.dtype)
    for k in env:
        monkeypatch.delenv(k)
    return eng


def _cmp(fam, got, ref, what):
    if fam.dtype == "f16":
        _close(got, ref, **{**dict(rel=2e-3, abs_=1e-3), **fam.tol})
    else:
        _close32(got, ref, what)


def _schedule(eng, n):
    return [(p["layer"], p["op"], p["tile"]) for p in eng.profile(n, 1)]


def _is_fused(p):
    return p["op"] >= 100 or p["tile"] // 1000000 == 37 or bool(sig_sep32([p]))


def _launch_of(prof, layer):
    """The profile row (its first layer) that runs `layer`: its own row, or - for a layer a fused launch swallowed - the fused row right in
    front of it (only rowless layers in between), or else the next fused row behind it (a bottleneck's projection and own reduction sit in
    front of the row that runs them).  None: no fused row claims it."""
    rows = {p["layer"]: p for p in prof}
    if layer in rows:
        return layer
    j = layer
    while j >= 0 and j not in rows:
        j -= 1
    if j >= 0 and _is_fused(rows[j]):
        return j
    later = [q for q in sorted(rows) if q > layer and _is_fused(rows[q])]
    return later[0] if later else None


def check_case(monkeypatch, fam, g, want=None):
    """Everything the module docstring lists, for one built graph; `want` = None: no fired / refused expectation (composition graphs)."""
    net, n, f16 = g.net, g.n, fam.dtype == "f16"
    frames = _frames(n, g.h, g.w, seed=fam.seed + n)
    ref, tens = ref_net.run(net.layers, g.outs, net.blob(), frames_u8=frames, match_fp16=f16, return_tensors=True)
    eng = _engine(monkeypatch, g, fam, fam.env)
    got = eng.inference(frames)
    footprint.assert_zero_outside(eng, footprint.tensor_ids(net.layers), n, fam.name)
    prof = eng.profile(n, 1)
    fired = fam.sig(prof)
    print(f"{fam.name} {_pid(g.P if g.P[0] else None)}: fired {fired}, expected {want}")
    problems = []
    if want is not None and fired != want:
        problems.append(f"fused launches {fired}, expected {want}")
    # oracle
    names = sorted(ref)
    for b in range(n):
        assert [nm for nm, _ in got[b]] == names
        for nm, arr in got[b]:
            try:
                if f16:
                    _check([[(nm, arr)]], {nm: ref[nm][b:b + 1]}, 1, **{**dict(rel=2e-3, abs_=1e-3), **fam.tol})
                else:
                    _close32(arr, ref[nm][b], nm)
            except AssertionError as e:
                problems.append(f"oracle, output {nm} frame {b}: {e}")
    if not f16:
        assert eng.split_fallbacks == 0
    # every live tensor
    for t in range(1, net.nt):
        if t not in tens:
            continue
        readers = [i for i, L in enumerate(net.layers) if L.in_ == t or L.res == t]
        named = [o for o in g.outs if o.tensor == t]
        try:
            mine = eng.debug_tensor(t, n)
        except _lib.HpError as e:
            msg = str(e)
            if "arena" in msg:
                continue            # fp32: shares its buffer with later tensors - only its readers' results can be checked
            if "fp32 network output" in msg:
                ok = not readers and named
            else:   # elided: every reader runs in the launch that swallowed the layer(s) writing it, in the same pattern
                writers = [i for i, L in enumerate(net.layers) if L.out == t]
                home = {_launch_of(prof, i) for i in writers}
                ok = (not named and len(home) == 1 and None not in home and all(_launch_of(prof, i) in home for i in readers)
                      and all(i in g.inside and g.seg_of[i] == g.seg_of.get(writers[0]) for i in readers))
            if not ok:
                problems.append(f"tensor {t} is not materialised ({msg}) but layers {readers} / outputs {[o.name for o in named]} read it")
            continue
        try:
            _cmp(fam, mine, tens[t][:n], f"tensor {t}")
        except AssertionError as e:
            problems.append(f"live tensor {t}: {e}")
    # per-layer schedule
    eng2 = _engine(monkeypatch, g, fam, fam.off)
    got2 = eng2.inference(frames)
    assert not fam.sig(eng2.profile(n, 1))
    same = _schedule(eng, n) == _schedule(eng2, n)
    for b in range(n):
        for (nm, a), (_, a2) in zip(got[b], got2[b]):
            if same or fam.xbits or (getattr(fam, "bits_if", None) and fam.bits_if(prof)):
                if not np.array_equal(a, a2):
                    problems.append(f"per-layer schedule, output {nm} frame {b}: bits differ (max {np.abs(a - a2).max():.4g})")
            else:
                try:
                    _close(a, a2, **fam.xtol)
                except AssertionError as e:
                    problems.append(f"per-layer schedule, output {nm} frame {b}: {e}")
    # a switch that only changes how the launches are issued: same bits
    if fam.ab:
        got3 = _engine(monkeypatch, g, fam, {**fam.env, **fam.ab}).inference(frames)
        for b in range(n):
            for (nm, a), (_, a3) in zip(got[b], got3[b]):
                if not np.array_equal(a, a3):
                    problems.append(f"{fam.ab}, output {nm} frame {b}: bits differ (max {np.abs(a - a3).max():.4g})")
    # batch invariance
    alone = eng.inference(frames[n - 1:n])[0]
    for (nm, a1), (_, ab) in zip(alone, got[n - 1]):
        if not np.array_equal(a1, ab):
            problems.append(f"batch invariance, output {nm}")
    assert not problems, "\n".join(problems)
    return fired


def _guarded(run):
    """A failed HIP call (HP_ERR_HIP: a launch the runtime refused, a fault) ends the session: nothing more is started on that device."""
    try:
        run()
    except _lib.HpError as e:
        if e.code == -2:
            pytest.exit(f"a HIP call failed, stopping: {e}", returncode=3)
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("family,P,want", CASES)
def test_fusion_pass_on_perturbed_graph(hp, monkeypatch, family, P, want):
    fam = FAMILIES[family]
    _guarded(lambda: check_case(monkeypatch, fam, build(fam, P), want))


@pytest.mark.gpu
def test_depthwise_without_a_kernel_is_refused_when_built(hp):
    """What the per-layer schedule cannot run either is an error of hp_engine_create, not of the first inference: a depthwise layer at
    stride 2 with dilation 2 (dwconv3x3_kernel's halo tile has no such form), with PReLU, or with a residual (no depthwise / pooling kernel
    adds one - it used to be dropped without a word)."""
    for kw in (dict(stride=2, dil=2), dict(act=PRELU), dict(res=1)):
        net = Net(5)
        a = net.conv(0, 3, 64, 3, 1)
        d = net.conv(a, 64, 64, 3, op=DW, **{**dict(act=RELU6), **kw})
        y = net.conv(d, 64, 128, 1)
        with pytest.raises(_lib.HpError):
            E.Engine(net.layers, [Out("y", y, 0, 128).c()], net.blob(), 27, 23, 2)


# ---------------------------------------------------------------- pass interaction
def _segments():
    """Patterns that take a 128-channel trunk and hand one on, with the perturbations that keep it so."""
    def sep(g, x):
        return pat_sep(128, 128)(g, x)[0]

    def chain2(g, x):
        return pat_chain2(g, x)[0]

    def chain3(g, x):
        return pat_chain3(g, x)[0]

    def head(g, x):          # a side branch: the trunk goes on
        y = pat_head(g, x)[0]
        g.outs.append(Out(f"h{len(g.outs)}", y.t, y.coff, y.c))
        return x

    def bneck(g, x):         # 128 -> 256 (a launch of its own) -> bottleneck M = 64 -> the next block's reduction to 128 channels
        up = g.add(x, 256, 1)
        r = g.add(up, 64, 1)
        v = g.layer(0, r, 64, 3)
        y = g.layer(1, v, 256, 1, res=up, rba=1)
        return g.layer(2, y, 128, 1, last=True)

    acts = [("act", i, a, p) for i in (0, 1) for a, p in ((NONE, 0.0), (LEAKY, 0.1), (LEAKY, 0.0), (RELU6, 0.0))]
    common = [None, ("reader", 0), ("mid_out", 0, 0.0), ("mid_out", 0, 2.0), ("between", 1), ("out_coff", 8), ("out_coff", 32), ("outs", "sub"), ("outs", "twice")]
    return [(sep, common + acts + [("geom", 0, "dil2"), ("geom", 0, "pads")]),
            (chain2, common + acts + [("as_res", 0), ("geom", 1, "dil2"), ("geom", 0, "pads")]),
            (chain3, common + acts + [("reader", 1), ("act", 2, NONE, 0.0), ("res", 2, "flip"), ("res", 2, "none"), ("between", 2)]),
            (head, [None, ("reader", 0), ("act", 0, RELU6, 0.0), ("act", 0, NONE, 0.0), ("act", 1, LEAKY, 0.1), ("between", 1), ("out_coff", 8)]),
            (bneck, [None, ("reader", 0), ("act", 2, NONE, 0.0), ("act", 0, RELU6, 0.0), ("between", 2), ("between", 1), ("res", 1, "flip"), ("out_coff", 8), ("outs", "sub")])]


def build_composition(seed, given=None):
    """Built twice like every case: what the perturbations need next to their patterns is written behind the stem, not inside a pattern."""
    rng = np.random.default_rng(seed)
    segs = _segments()
    g = G(seed, (13 * 4, 17 * 4), None, given)
    t = g.add(None, 32, 3, 2)
    x = g.add(t, 128, 3, 2)
    g.refs["x"] = x
    g.stem_done(x)
    picks = []
    for s in range(int(rng.integers(3, 6))):
        pat, perts = segs[int(rng.integers(len(segs)))]
        P = perts[int(rng.integers(len(perts)))]
        picks.append((pat.__name__, P))
        g.P, g.refs, g.seg = P or (None,), {"x": x}, s
        first_out = len(g.outs)
        y = pat(g, x)
        g.finish([y] if y is not x else [], tail=False)
        for o in g.outs[first_out:]:     # one name per segment
            o.name = f"s{s}_{o.name.decode()}".encode()
        x = Ref(y.t, y.coff, y.c)
        g.refs["x"] = x
    g.P = (None,)
    z = g.add(x, 32, 1, act=NONE)
    g.outs.append(Out("z", z.t, 0, 32))
    g.picks = picks
    if given is None and g.want:
        return build_composition(seed, g.want)
    return g


def composition_family(g):
    """The bounds of the families in the graph, none wider: 2e-3 of scale + 1e-3 against the oracle and across schedules (separable blocks,
    chains, heads), 3e-3 + 1e-3 and 4e-3 + 2e-3 where a bottleneck is one of the patterns (test_bottleneck_variants).  Where the fused engine's
    only fused launches are separable blocks the two schedules must agree bit for bit (check_case: `bits_if`)."""
    bneck = any(name == "bneck" for name, _ in g.picks)
    fam = Family("composition", None, None, lambda prof: [p["tile"] for p in prof if p["op"] >= 100], (13, 17), down=4,
                 tol=dict(rel=3e-3) if bneck else {}, xtol=dict(rel=4e-3, abs_=2e-3) if bneck else dict(rel=2e-3, abs_=1e-3))
    fam.bits_if = lambda prof: all(p["op"] in (100,) for p in prof if p["op"] >= 100)
    return fam


COMPOSITION_SEEDS = [3, 7, 11, 19, 23, 31, 42, 57, 64, 77, 89, 101]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", COMPOSITION_SEEDS)
def test_fusion_passes_in_sequence(hp, monkeypatch, seed):
    """3 - 5 patterns behind each other on one 128-channel trunk, each with one random perturbation (seeded): a chain behind a separable
    block, a head next to a chain, a bottleneck whose "next reduction" is the trunk of the following pattern ... - the same oracle, live-tensor,
    per-layer-schedule and batch assertions at the families' own bounds (composition_family), and at least one fused launch per graph."""
    g = build_composition(seed)
    print(seed, g.picks)
    fired = []
    _guarded(lambda: fired.extend(check_case(monkeypatch, composition_family(g), g)))
    assert fired, "every pattern of the graph was refused: no pass interaction exercised"


@pytest.mark.gpu
def test_compositions_reach_every_pass(hp, monkeypatch):
    """Over the seeds, the fused engines launch separable blocks, heads, chains and bottlenecks (engines built and profiled, nothing else)."""
    ops = set()
    for seed in COMPOSITION_SEEDS:
        g = build_composition(seed)
        eng = _engine(monkeypatch, g, composition_family(g), {})
        ops |= {p["op"] for p in eng.profile(g.n, 1) if p["op"] >= 100}
    assert ops == {100, 101, 102, 103}, ops


# ---------------------------------------------------------------- CPU twin
def _well_formed(g, what):
    frames = _frames(g.n, g.h, g.w, seed=1)
    shapes = g.expected_shapes()
    assert len(shapes) == len(g.outs), (what, "duplicate output names")
    for match in (True, False):
        ref = ref_net.run(g.net.layers, g.outs, g.net.blob(), frames_u8=frames, match_fp16=match)
        for nm, arr in ref.items():
            assert arr.shape == shapes[nm], (what, nm, arr.shape, shapes[nm])
            assert np.isfinite(arr).all() and arr.std() > 0, (what, nm)


@pytest.mark.parametrize("family", list(ROWS))
def test_graph_cases_are_well_formed(family):
    """No GPU: every case of the family evaluates on the oracle (both fp16 settings) to finite, non-constant outputs of the expected shapes,
    and the table is not vacuous - the canonical case fires, at least three perturbed cases fire and at least three are refused."""
    fam, rows = FAMILIES[family], ROWS[family]
    assert len({_pid(P) for P, _, _ in rows}) == len(rows), "duplicate rows"
    assert rows[0][0] is None and rows[0][1], "the canonical case must fire"
    canonical = rows[0][1]
    assert sum(1 for P, want, _ in rows if P is not None and want == canonical) >= 3
    if family in PARTIAL_IS_REFUSAL:
        assert sum(1 for P, want, _ in rows if want != canonical) >= 3
    else:
        assert sum(1 for P, want, _ in rows if want == []) >= 3, "at least three rows must run the per-layer schedule"
    for P, _, _ in rows:
        _well_formed(build(fam, P), (family, P))


def test_composition_graphs_are_well_formed():
    kinds = set()
    for seed in COMPOSITION_SEEDS:
        g = build_composition(seed)
        assert 3 <= len(g.picks) <= 5
        kinds |= {name for name, _ in g.picks}
        _well_formed(g, ("composition", seed, g.picks))
    assert kinds == {"sep", "chain2", "chain3", "head", "bneck"}
