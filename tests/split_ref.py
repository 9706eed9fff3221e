"""The split engine's arithmetic contract (HP_DTYPE_F32S, csrc/conv32_direct.hip), stated once in numpy - no kernel is involved.

The split.  x = hi + 2^-11 lo + r with hi = fp16(x), lo = fp16((x - hi) * 2^11), both computed in float32 as the staging code and the host's
weight packer do.  x - hi is exact in float32 (|x - hi| <= half an fp16 ulp of x, a multiple of x's own float32 ulp), and so is the
multiplication by 2^11 (no overflow: in the top binade |x - hi| <= 16, so |t| <= 32768 for t = (x - hi) 2^11).  What is lost is the fp16 rounding
of t alone:
  * t in fp16's normal range, x in [2^e, 2^(e+1)): |t| <= 2^e, and |t| = 2^e is a representable value, so a ROUNDED t lies below 2^e, where half an
    ulp is 2^(e-12): |r| <= 2^-11 2^(e-12) = 2^(e-23) <= 2^-23 |x|;
  * t an fp16 subnormal (|t| < 2^-14, a grid of 2^-24): |r| <= 2^-11 2^-25 = 2^-36 - the header's "ABSOLUTE error of 2^-36".
Hence |r| <= rho(x) = max(2^-23 |x|, 2^-36).  (|x| < 2^-25 gives hi = 0; |x| < 2^-36 gives lo = 0 as well: the bound still holds.)

One product.  The kernel forms P = hi_a hi_w + 2^-11 (hi_a lo_w + lo_a hi_w), every product exact in the matrix pipe's fp32 accumulator (two
11-bit significands).  With A = hi_a + 2^-11 lo_a = a - r_a and W likewise, P = A W - 2^-22 lo_a lo_w, so
    a w - P = a r_w + r_a w - r_a r_w + (2^-11 lo_a)(2^-11 lo_w),     |2^-11 lo_x| = |x - hi_x - r_x| <= |x - fp16(x)| + rho(x) = d(x):
    |a w - P| <= |a| rho(w) + rho(a) |w| + d(a) d(w) + rho(a) rho(w) = product_bound(a, w).
A zero operand splits into (0, 0) and its product is exactly zero: such terms carry no bound.

One output element with n non-zero terms.  acc0 = the fp32 sum of the n exact hi-hi products, acc1 = the fp32 sum of the 2 n exact cross products,
the epilogue forms fma(acc1, 2^-11, acc0) (one rounding) and adds the bias (one rounding).  In the standard model (every fp32 addition rounded to
nearest, ANY order, u = 2^-24) acc0 carries <= n - 1 roundings, acc1 <= 2 n - 1, and for fp16-normal operands |hi| <= (1 + 2^-11) |x| and
|2^-11 lo| <= 2^-11 (1 + 2^-11) |x|.  To first order, with S' = sum |a_i w_i| and S = S' + |bias|:
    (n - 1) u (1 + 2^-10) S'  +  (2 n + 1) u 2^-10 (1 + 2^-10) S'  +  2 u S   <=   (n + 1 + 3 n 2^-10 + 2^-9) u S   <=   (n + 2) u S   for n <= 330
and the (k u) / (1 - k u) form with k = n + 4 covers the higher-order terms with two roundings to spare.  For n = 1 acc0 is ONE exact product (no
rounding at all, whatever the operands' range): 3 roundings.  For n > 1 the derivation needs fp16-normal operands (|x| >= 2^-14) - layer_bound
refuses anything else, and anything beyond n = 330.
    layer_bound = sum of the product bounds + (n + 4) u / (1 - (n + 4) u) * S.

Layers are written as matrices: A [P, K] = one row of K operands per output pixel (patches() lays a SAME-padded NCHW tensor out that way, K in the
blob's (ky, kx, cin) order), Wt [K, C] = one column per output channel.  product_bound is separable, so the bound of a layer is four matrix
products.  The float64 sums here (exact(), emulate()) carry K 2^-53 of relative error: nothing next to 2^-24.
"""
import numpy as np

U = 2.0 ** -24
F16_MAX = 65504.0


def f32(x):
    return np.ascontiguousarray(x, np.float32)


def split(x):
    """(hi, lo) as float16 arrays: float32 arithmetic, round-to-nearest-even conversions with fp16 subnormals - the kernel's staging code."""
    x = f32(x)
    hi = x.astype(np.float16)
    lo = ((x - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    return hi, lo


def rho(x):
    return np.maximum(np.abs(np.asarray(x, np.float64)) * 2.0 ** -23, 2.0 ** -36)


def d(x):
    x = f32(x)
    return np.abs(x.astype(np.float64) - x.astype(np.float16).astype(np.float64)) + rho(x)


def product_bound(a, w):
    """|a w - (hi_a hi_w + 2^-11 (hi_a lo_w + lo_a hi_w))| for non-zero a, w (elementwise, float64)."""
    aa, ww = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(w, np.float64))
    return aa * rho(w) + rho(a) * ww + d(a) * d(w) + rho(a) * rho(w)


def _flush(h):
    """fp16 subnormals -> 0 (a mutant: a conversion or a matrix pipe that does not keep them)."""
    return np.where(np.abs(h.astype(np.float32)) < 2.0 ** -14, np.float16(0), h)


MUTANTS = ("drop_hi_lo", "drop_lo_hi", "drop_lo", "flush", "scale_2^-10")


def parts(x, mutant=None):
    hi, lo = split(x)
    if mutant == "flush":
        hi, lo = _flush(hi), _flush(lo)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate_product(a, w, mutant=None):
    """The split product of two scalars / arrays, elementwise, exact in float64 (every term has <= 22 significant bits)."""
    ha, la = parts(a, mutant)
    hw, lw = parts(w, mutant)
    c1 = 0.0 if mutant in ("drop_hi_lo", "drop_lo") else ha * lw
    c2 = 0.0 if mutant in ("drop_lo_hi", "drop_lo") else la * hw
    return ha * hw + (2.0 ** -10 if mutant == "scale_2^-10" else 2.0 ** -11) * (c1 + c2)


def emulate(A, Wt, bias=None, mutant=None):
    """A layer's outputs [P, C] under the contract (or a mutant of it), sums in float64."""
    ha, la = parts(A, mutant)
    hw, lw = parts(Wt, mutant)
    c1 = 0.0 if mutant in ("drop_hi_lo", "drop_lo") else ha @ lw
    c2 = 0.0 if mutant in ("drop_lo_hi", "drop_lo") else la @ hw
    out = ha @ hw + (2.0 ** -10 if mutant == "scale_2^-10" else 2.0 ** -11) * (c1 + c2)
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :]


def exact(A, Wt, bias=None):
    out = f32(A).astype(np.float64) @ f32(Wt).astype(np.float64)
    return out if bias is None else out + np.asarray(bias, np.float64)[None, :]


def layer_bound(A, Wt, bias=None):
    """The bound of every output element [P, C] (see the module's docstring); n = its number of non-zero terms."""
    A, Wt = f32(A), f32(Wt)
    za, zw = (A != 0).astype(np.float64), (Wt != 0).astype(np.float64)
    n = za @ zw
    if n.max() > 1:
        small = min(np.abs(A[A != 0]).min(), np.abs(Wt[Wt != 0]).min())
        if small < 2.0 ** -14 or n.max() > 330:
            raise ValueError("layer_bound: sums of more than one term are derived for fp16-normal operands and n <= 330")
    aa, ww = np.abs(A.astype(np.float64)), np.abs(Wt.astype(np.float64))
    prod = aa @ (rho(Wt) * zw) + (rho(A) * za) @ ww + (d(A) * za) @ (d(Wt) * zw) + (rho(A) * za) @ (rho(Wt) * zw)
    S = aa @ ww
    if bias is not None:
        S = S + np.abs(np.asarray(bias, np.float64))[None, :]
    k = (n + 4) * U
    return prod + k / (1 - k) * S


def patches(x, k):
    """NCHW [N, C, H, W] -> [N H W, k k C]: the operands of every output pixel of a k x k stride-1 SAME convolution, (ky, kx, c) order."""
    x = f32(x)
    N, C, H, W = x.shape
    p = (k - 1) // 2
    xp = np.zeros((N, C, H + 2 * p, W + 2 * p), np.float32)
    xp[:, :, p:p + H, p:p + W] = x
    cols = [xp[:, :, ky:ky + H, kx:kx + W].transpose(0, 2, 3, 1) for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=3).reshape(N * H * W, k * k * C)


def as_nchw(out, N, H, W):
    """[N H W, C] -> [N, C, H, W]."""
    return out.reshape(N, H, W, -1).transpose(0, 3, 1, 2)


# ---------------------------------------------------------------- input designs (shared by the CPU sensitivity test and the GPU tests)
N, H, W = 2, 13, 11                     # 2 x 13 x 11 frames: ragged 8 x 8 blocks
# Binades [2^e, 2^(e+1)), both ends inclusive; "top" is clipped to 65504.  "straddle" is the VALUE range [2^-13, 2^-11) around 2^-12, the two
# binades where a quarter to a half of all lo parts are fp16 subnormals: with the binade of 2^-11 drawn as well, flushed subnormals left
# layer_bound on only 0.47 - 0.54 of the outputs (tests/test_split_contract_cpu.py asks for half): the design changed, not the threshold
WINDOWS = {"tiny": (-30, -13), "straddle": (-13, -12), "unit": (-6, 2), "top": (10, 15)}
RUNS = [("tiny", "tiny"), ("straddle", "straddle"), ("unit", "unit"), ("top", "top"), ("tiny", "unit"), ("unit", "tiny")]   # (activations, weights)
SHAPES = [(64, 128, 3), (128, 512, 1), (64, 19, 1)]    # (cin, cout, k): the split instances 33003 / 33001 of test_engine_footprint_gpu.py


def significands(rng, shape):
    """+-[1, 2) with all 23 fraction bits random."""
    m = (1.0 + rng.integers(0, 2 ** 23, shape).astype(np.float64) * 2.0 ** -23).astype(np.float32)
    return m * rng.choice(np.float32([-1, 1]), shape)


class OneTap:
    """Part 1.  Frames of full significands in +-[1, 2); a first layer 1 x 1, 3 -> cin with ONE power-of-two weight per output channel
    (activation c = plane c % 3 times 2^e_c, exact); the layer under test with ONE non-zero weight per output channel at a tap and an input
    channel that vary with the channel.  Both exponents are drawn from their windows; the top window is clipped to 65504."""

    def __init__(self, cin, cout, k, act_win, w_win, seed=0):
        rng = np.random.default_rng([seed, cin, cout, k, list(WINDOWS).index(act_win), list(WINDOWS).index(w_win)])
        self.cin, self.cout, self.k = cin, cout, k
        lo, hi = WINDOWS[act_win]
        self.frames = significands(rng, (N, 3, H, W))
        if act_win == "top":
            self.frames = np.clip(self.frames, -np.float32(F16_MAX / 2 ** 15), np.float32(F16_MAX / 2 ** 15))
        self.e_act = rng.integers(lo, hi + 1, cin)
        self.w_first = np.zeros((cin, 3), np.float32)                       # [cout][1][1][3]
        self.w_first[np.arange(cin), np.arange(cin) % 3] = np.float32(2.0) ** self.e_act
        self.act = self.frames[:, np.arange(cin) % 3] * (np.float32(2.0) ** self.e_act)[None, :, None, None]   # exact
        lo, hi = WINDOWS[w_win]
        co = np.arange(cout)
        self.ky, self.kx, self.ci = co % k, (co // k) % k, (co * 7 + 3) % cin
        val = np.ldexp(significands(rng, cout).astype(np.float64), rng.integers(lo, hi + 1, cout)).astype(np.float32)
        if w_win == "top":
            val = np.clip(val, -np.float32(F16_MAX), np.float32(F16_MAX))
        self.w = np.zeros((cout, k, k, cin), np.float32)                    # the blob's layout
        self.w[co, self.ky, self.kx, self.ci] = val
        self.Wt = self.w.reshape(cout, -1).T.copy()
        assert np.abs(self.act).max() <= F16_MAX and np.abs(self.w).max() <= F16_MAX


def aligned(rng, shape, lo, hi):
    """Positive h + r, h an fp16 number in [lo, hi), r between 0.05 and 0.45 fp16 ulps of h: every lo of the split is positive."""
    h = rng.uniform(lo, hi, shape).astype(np.float16)
    x = (h.astype(np.float64) + rng.uniform(0.05, 0.45, shape) * np.spacing(h).astype(np.float64)).astype(np.float32)
    hi_, lo_ = split(x)
    assert np.array_equal(hi_, h) and (lo_ > 0).all()
    return x


class Aligned:
    """Part 2.  Positive operands with aligned remainders: frames in [1, 2), first-layer weights 2^e_c with e_c in {-1, 0, 1}, dense weights in
    [2^-5, 2^-3), biases in [0.1, 1).  `dw`: a depthwise 3 x 3 (weights in [2^-6, 2^-4), RELU6 never clamps) sits between the two."""

    def __init__(self, cin, cout, k, dw=False, seed=0):
        rng = np.random.default_rng([seed, cin, cout, k, int(dw)])
        self.cin, self.cout, self.k, self.dw = cin, cout, k, dw
        self.frames = aligned(rng, (N, 3, H, W), 1.0, 2.0)
        self.e_act = rng.integers(-1, 2, cin)
        self.w_first = np.zeros((cin, 3), np.float32)
        self.w_first[np.arange(cin), np.arange(cin) % 3] = np.float32(2.0) ** self.e_act
        self.act = self.frames[:, np.arange(cin) % 3] * (np.float32(2.0) ** self.e_act)[None, :, None, None]
        self.w = aligned(rng, (cout, k, k, cin), 2.0 ** -5, 2.0 ** -3)
        self.Wt = self.w.reshape(cout, -1).T.copy()
        self.bias = aligned(rng, cout, 0.1, 1.0)
        if dw:
            self.dw_w = aligned(rng, (cin, 3, 3), 2.0 ** -6, 2.0 ** -4)     # [c][ky][kx], the blob's layout
            self.dw_b = aligned(rng, cin, 0.1, 0.5)

    def depthwise(self, x):
        """The depthwise layer on NCHW float32 x in the kernel's own order: bias first, then fmaf over the taps in (ky, kx) order, RELU6.  Each
        fmaf is a float64 product (exact) and sum, rounded to float32: the double rounding can differ from a true fmaf by one float32 ulp in
        about 2^-29 of the operations - 2^-24 of ONE of 64 terms, far inside layer_bound."""
        x = f32(x)
        n, c, h, w = x.shape
        xp = np.zeros((n, c, h + 2, w + 2), np.float32)
        xp[:, :, 1:-1, 1:-1] = x
        acc = np.broadcast_to(self.dw_b[None, :, None, None], x.shape).astype(np.float32)
        for ky in range(3):
            for kx in range(3):
                t = xp[:, :, ky:ky + h, kx:kx + w].astype(np.float64) * self.dw_w[None, :, ky, kx, None, None].astype(np.float64)
                acc = (t + acc.astype(np.float64)).astype(np.float32)
        assert acc.min() > 0 and acc.max() < 6
        return acc
