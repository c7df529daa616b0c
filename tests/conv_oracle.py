"""numpy fp64 oracle of the partial convolution as the C ABI defines it (include/terragan_hip.h: tg_conv_fwd, tg_conv_dgrad,
tg_conv_wgrad and their BatchNorm-on-load forms), independent of the package: nothing here imports tg_hip, torch or oracle/.

Layouts are the kernels': activations NHWC, weights [Cout][k][k][Cin], masks and ratios [B][H][W].

    forward   y  = act((conv(xin (.) m, W) + b) * ratio),   xin = x, or act_bn(((x - mean) * rstd) * gamma + beta)  (BN-on-load)
    dgrad     dx = convT(dy, W) (.) m * act'(gate) (+ base)
    wgrad     dW = sum_pix dy (x) (xin (.) m),   db = sum_pix dy

Every function returns a `Res`: next to the value, per output element, S = sum |a| |b| over its products (+ |bias|), K = the
number of products, `scale` = the factor the epilogue multiplies the sum by, and `base` = |accumulate base|.  From these
`bound()` gives the a-priori error bound of ANY fp32 evaluation of that element, whatever its summation order, tile shape or
split-K plan (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1: a sum of n products evaluated in any
order with or without fused multiply-adds errs by at most n u sum |a_i b_i| to first order, u = 2^-24):

    |fp32_i - ref_i| <= n_i * 2^-24 * (S_i * |scale_i| + base_i),   n_i = K_i + slabs + 4 (+ 4 under BN-on-load)

`slabs` = the most partial sums the route can add on top (split-K slabs, partial slabs of a persistent grid); the 4 pay for the
bias add, the ratio / mask multiply, the activation's slope and the accumulate add; the 4 under BN-on-load for the three
roundings of (x - mean) * rstd * gamma + beta, for which S is built from |(x - mean) rstd gamma| + |beta| in place of |xin|.
ReLU and LeakyReLU are 1-Lipschitz, so the bound of the pre-activation holds for the output.

With small-integer data every product and partial sum is an integer; where max S < 2^24 (`exact_ok`) every fp32 evaluation is
exact and must equal the reference bit for bit."""
from collections import namedtuple

import numpy as np

ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2
U = 2.0 ** -24
EXACT_LIMIT = 2.0 ** 24

Res = namedtuple("Res", "val S K scale base bn")


def f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def act(v, kind, slope=0.0):
    if kind == ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if kind == ACT_LEAKY:
        return np.where(v > 0, v, v * slope)
    return v


def act_grad(gate, kind, slope=0.0):
    """act'(.) as the kernels take it from an activation OUTPUT: 1 where it is positive, else the slope (0 for ReLU)."""
    if kind == ACT_NONE:
        return np.ones_like(gate)
    return np.where(gate > 0, 1.0, slope if kind == ACT_LEAKY else 0.0)


def out_size(n, k, s, p):
    return (n + 2 * p - k) // s + 1


def _source(x, mask, in_bn):
    """(xin (.) m, an upper bound of its magnitude that the rounding analysis may use)."""
    x = f64(x)
    if in_bn is not None:
        mean, rstd, gamma, beta = (f64(t) for t in in_bn[:4])
        a_kind = in_bn[4] if len(in_bn) > 4 else ACT_RELU
        a_slope = in_bn[5] if len(in_bn) > 5 else 0.0
        lin = (x - mean) * rstd * gamma
        xin, xabs = act(lin + beta, a_kind, a_slope), np.abs(lin) + np.abs(beta)
    else:
        xin, xabs = x, np.abs(x)
    if mask is not None:
        m = f64(mask)[..., None]
        xin, xabs = xin * m, xabs * np.abs(m)
    return xin, xabs


def _pad(a, p):
    return np.pad(a, ((0, 0), (p, p), (p, p), (0, 0))) if p else a


def _taps(k, s, Ho, Wo):
    for ky in range(k):
        for kx in range(k):
            yield ky, kx, (slice(None), slice(ky, ky + s * (Ho - 1) + 1, s), slice(kx, kx + s * (Wo - 1) + 1, s), slice(None))


def conv_fwd(x, w, k, s, p, mask=None, bias=None, ratio=None, act_kind=ACT_NONE, slope=0.0, in_bn=None):
    w = f64(w)
    B, H, W, Cin = np.shape(x)
    Cout = w.shape[0]
    assert w.shape == (Cout, k, k, Cin), (w.shape, Cout, k, Cin)
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    xin, xabs = _source(x, mask, in_bn)
    xin, xabs = _pad(xin, p), _pad(xabs, p)
    inside = _pad(np.ones((1, H, W, 1)), p)
    z = np.zeros((B, Ho, Wo, Cout))
    S = np.zeros((B, Ho, Wo, Cout))
    K = np.zeros((1, Ho, Wo, 1))
    wabs = np.abs(w)
    for ky, kx, sl in _taps(k, s, Ho, Wo):
        z += xin[sl] @ w[:, ky, kx, :].T
        S += xabs[sl] @ wabs[:, ky, kx, :].T
        K += inside[sl] * Cin
    if bias is not None:
        z = z + f64(bias)
        S = S + np.abs(f64(bias))
    scale = np.ones((B, Ho, Wo, 1))
    if ratio is not None:
        z = z * f64(ratio)[..., None]
        scale = np.abs(f64(ratio))[..., None]
    return Res(act(z, act_kind, slope), S, np.broadcast_to(K, S.shape), np.broadcast_to(scale, S.shape), np.zeros_like(S),
               in_bn is not None)


def conv_dgrad(dy, w, x_shape, k, s, p, mask=None, gate=None, gate_act=ACT_RELU, gate_slope=0.0, base=None):
    dy, w = f64(dy), f64(w)
    B, H, W, Cin = x_shape
    Cout = w.shape[0]
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    assert dy.shape == (B, Ho, Wo, Cout) and w.shape == (Cout, k, k, Cin), (dy.shape, w.shape)
    dx = np.zeros((B, H + 2 * p, W + 2 * p, Cin))
    S = np.zeros_like(dx)
    K = np.zeros((1, H + 2 * p, W + 2 * p, 1))
    dyabs, wabs = np.abs(dy), np.abs(w)
    for ky, kx, sl in _taps(k, s, Ho, Wo):
        dx[sl] += dy @ w[:, ky, kx, :]
        S[sl] += dyabs @ wabs[:, ky, kx, :]
        K[sl] += Cout
    crop = (slice(None), slice(p, p + H), slice(p, p + W), slice(None))
    dx, S, K = dx[crop], S[crop], K[crop]
    scale = np.ones((B, H, W, Cin))
    if mask is not None:
        scale = scale * f64(mask)[..., None]
    if gate is not None:
        scale = scale * act_grad(f64(gate), gate_act, gate_slope)
    dx = dx * scale
    b0 = np.zeros_like(dx)
    if base is not None:
        dx = dx + f64(base)
        b0 = np.abs(f64(base))
    return Res(dx, S, np.broadcast_to(K, S.shape), np.abs(scale), b0, False)


def conv_wgrad(x, dy, k, s, p, mask=None, in_bn=None):
    """(dW as [Cout][k][k][Cin], db)."""
    dy = f64(dy)
    B, H, W, Cin = np.shape(x)
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    Cout = dy.shape[3]
    assert dy.shape == (B, Ho, Wo, Cout), dy.shape
    xin, xabs = _source(x, mask, in_bn)
    xin, xabs = _pad(xin, p), _pad(xabs, p)
    inside = _pad(np.ones((1, H, W, 1)), p)
    dw = np.zeros((Cout, k, k, Cin))
    S = np.zeros_like(dw)
    K = np.zeros((1, k, k, 1))
    d2, d2abs = dy.reshape(-1, Cout).T, np.abs(dy).reshape(-1, Cout).T
    for ky, kx, sl in _taps(k, s, Ho, Wo):
        dw[:, ky, kx, :] = d2 @ xin[sl].reshape(-1, Cin)
        S[:, ky, kx, :] = d2abs @ xabs[sl].reshape(-1, Cin)
        K[0, ky, kx, 0] = B * inside[sl].sum()
    one = np.ones_like(S)
    rw = Res(dw, S, np.broadcast_to(K, S.shape), one, np.zeros_like(S), in_bn is not None)
    Sb = np.abs(dy).sum(axis=(0, 1, 2))
    rb = Res(dy.sum(axis=(0, 1, 2)), Sb, np.full(Cout, float(B * Ho * Wo)), np.ones(Cout), np.zeros(Cout), False)
    return rw, rb


def bound(r, slabs):
    """The a-priori bound of the module docstring, per element."""
    n = r.K + slabs + 4 + (4 if r.bn else 0)
    return n * U * (r.S * r.scale + r.base)


def exact_ok(r):
    """Every partial sum of every element is an integer below 2^24 (given integer data): any fp32 order is exact."""
    return float((r.S * np.maximum(r.scale, 1.0) + r.base).max()) < EXACT_LIMIT


def worst(x, r, slabs):
    """max_i err_i / bound_i (0/0 = 0: an element whose bound is zero must be exact), and the flat index where it is reached."""
    x = f64(x)
    assert x.shape == r.val.shape, (x.shape, r.val.shape)
    if not np.isfinite(x).all():
        return float("inf"), -1
    e, b = np.abs(x - r.val), bound(r, slabs)
    q = np.where(e == 0, 0.0, e / np.where(b > 0, b, 1.0) + np.where(b > 0, 0.0, np.inf))
    i = int(q.argmax())
    return float(q.reshape(-1)[i]), i
