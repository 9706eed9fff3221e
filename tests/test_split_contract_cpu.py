"""CPU: the split engine's contract as tests/split_ref.py states it - the reference inside its own bound, and the gate of
tests/test_engine_ranges_gpu.py sharp on the very inputs it runs: every way of getting the split subtly wrong leaves layer_bound on at least
half of the output elements of every input design.  No kernel runs here; the conditions are conditions on inputs.
"""
import numpy as np
import pytest

import split_ref as S


def _window_operands(rng, win, count):
    lo, hi = S.WINDOWS[win]
    x = np.ldexp(S.significands(rng, count).astype(np.float64), rng.integers(lo, hi + 1, count)).astype(np.float32)
    return np.clip(x, -np.float32(S.F16_MAX), np.float32(S.F16_MAX))


@pytest.mark.parametrize("act_win,w_win", S.RUNS + [("straddle", "top"), ("top", "tiny")], ids=lambda v: v)
def test_the_emulation_stays_inside_product_bound(act_win, w_win):
    rng = np.random.default_rng([7, list(S.WINDOWS).index(act_win), list(S.WINDOWS).index(w_win)])
    a, w = _window_operands(rng, act_win, 400000), _window_operands(rng, w_win, 400000)
    err = np.abs(a.astype(np.float64) * w.astype(np.float64) - S.emulate_product(a, w))
    ratio = err / S.product_bound(a, w)
    print(f"{act_win} x {w_win}: worst |a w - P| / product_bound = {ratio.max():.4f}")
    assert (ratio <= 1).all()


def test_the_split_itself():
    """x = hi + 2^-11 lo + r with |r| <= rho(x), on every window, at the edges of fp16's range and below both grids."""
    rng = np.random.default_rng(3)
    x = np.concatenate([_window_operands(rng, win, 200000) for win in S.WINDOWS]
                       + [np.float32([65504, -65504, 65503.996, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -36, 2.0 ** -37, 1.5 * 2.0 ** -36, 0])])
    hi, lo = S.split(x)
    assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
    r = x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64) * 2.0 ** -11
    assert (np.abs(r) <= S.rho(x)).all()
    assert np.abs(lo.astype(np.float32)).max() == 32768           # the top binade: lo reaches 2^15


def _designs():
    for cin, cout, k in S.SHAPES:
        for aw, ww in S.RUNS:
            yield f"tap-{cin}-{cout}-{k}x{k}-{aw}-{ww}", (cin, cout, k, aw, ww)
    yield "sum-1x1-64", (64, 128, 1, False)
    yield "sum-3x3-32", (32, 64, 3, False)
    yield "sum-dw-1x1-64", (64, 128, 1, True)


DESIGNS = dict(_designs())


def _operands(key):
    spec = DESIGNS[key]
    if key.startswith("tap"):
        des = S.OneTap(*spec)
        return des, S.patches(des.act, des.k), des.Wt, None
    des = S.Aligned(*spec)
    x = des.depthwise(des.act) if des.dw else des.act
    return des, S.patches(x, des.k), des.Wt, des.bias


def _reaches_below_fp16_normal(A, Wt):
    """Whether the design has fp16-subnormal hi / lo parts at all: in a tenth of its non-zero operands on one side at least."""
    def share(x):
        x = x[x != 0]
        hi, lo = S.split(x)
        sub = lambda h: (np.abs(h.astype(np.float32)) < 2.0 ** -14) & (h != 0)   # noqa: E731
        return float((sub(hi) | sub(lo)).mean())
    return max(share(A), share(Wt)) >= 0.1


@pytest.mark.parametrize("key", list(DESIGNS))
def test_every_mutant_leaves_layer_bound_on_half_of_the_outputs(key):
    """The reference stays inside layer_bound on the design; each mutant - a cross term dropped (either one), lo dropped, fp16 subnormals
    flushed, 2^-10 for 2^-11 - exceeds it on >= half of ALL output elements (padding taps, which are exactly zero, included in the count).
    Flushing subnormals changes nothing where no operand has a subnormal part (the O(1) and top windows, the sums): there the mutant IS the
    contract, which is asserted instead - no design of those windows can separate the two."""
    des, A, Wt, bias = _operands(key)
    ref, bound = S.exact(A, Wt, bias), S.layer_bound(A, Wt, bias)
    good = np.abs(S.emulate(A, Wt, bias) - ref)
    assert (good <= bound).all(), float((good / np.maximum(bound, 1e-300)).max())
    for m in S.MUTANTS:
        bad = np.abs(S.emulate(A, Wt, bias, mutant=m) - ref)
        over = float((bad > bound).mean())
        ratio = float(np.median((bad / np.maximum(bound, 1e-300))[bound > 0]))
        print(f"{key} {m}: beyond layer_bound on {over:.3f} of the outputs, median error / bound {ratio:.3g}")
        if m == "flush" and not _reaches_below_fp16_normal(A, Wt):
            assert over <= 0.01
            continue
        assert over >= 0.5, (key, m, over)


def test_layer_bound_refuses_what_it_is_not_derived_for():
    a = np.full((1, 4), 2.0 ** -20, np.float32)
    with pytest.raises(ValueError):
        S.layer_bound(a, np.ones((4, 1), np.float32))
    with pytest.raises(ValueError):
        S.layer_bound(np.ones((1, 400), np.float32), np.ones((400, 1), np.float32))
