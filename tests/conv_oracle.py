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


def bf16_rne(a):
    """An fp32 array rounded to the nearest bf16, ties to even, as fp32 -- what the bf16 direct kernels do to the two MFMA operands
    when they stage them into LDS (igemm.hip: __builtin_convertvector f32x4 -> bf16x4 = v_cvt_pk_bf16_f32), and to nothing else.
    The bit form: add 0x7FFF plus the lowest kept bit, drop the low half.  A carry out of the mantissa moves the exponent, the
    largest finite values go to inf, subnormals round on the same grid.  (No NaN handling: the tables draw none.)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(a))


def bf16_trunc(a):
    """The fp32 array with the low 16 bits dropped: the WRONG conversion, which the rounded-operand run must tell from bf16_rne."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(np.float32).reshape(np.shape(a))


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


def conv_wgrad(x, dy, k, s, p, mask=None, in_bn=None, dy_bias=None):
    """(dW as [Cout][k][k][Cin], db).  `dy_bias`: the dy that db sums, where it is not the dW operand (bf16 mode rounds the MFMA
    operands; the bias gradient stays the fp32 column sum of the unrounded dy)."""
    dy, dyb = f64(dy), f64(dy if dy_bias is None else dy_bias)
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
    Sb = np.abs(dyb).sum(axis=(0, 1, 2))
    rb = Res(dyb.sum(axis=(0, 1, 2)), Sb, np.full(Cout, float(B * Ho * Wo)), np.ones(Cout), np.zeros(Cout), False)
    return rw, rb


def bound(r, slabs):
    """The a-priori bound of the module docstring, per element."""
    n = r.K + slabs + 4 + (4 if r.bn else 0)
    return n * U * (r.S * r.scale + r.base)


def exact_ok(r):
    """Every partial sum of every element is an integer below 2^24 (given integer data): any fp32 order is exact.  (A result of
    a Winograd route, WRes: the condition of its algorithm, wino_exact_ok.)"""
    if hasattr(r, "alg"):
        return wino_exact_ok(r)
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


# ---- the Winograd routes (csrc/wino.inc, wino16.inc, wino22.inc, wino44.inc) ---------------------------------------------------------
# A Winograd kernel does not add the products x w of the direct form: it adds, per transform point, products of TRANSFORMED operands,
# Y = At [ sum_k (G g_k Gt) (.) (Bt d_k B) ] A.  Its rounding errors are therefore bounded by the sum of absolute values of THAT
# expression,
#     S_w = |At| [ sum_k (|G| |g_k| |Gt|) (.) (|Bt| |d_k| |B|) ] |A|
# (every partial result of every transform pass and of the contraction is bounded in magnitude by the corresponding partial result
# of S_w, so the argument of the module docstring goes through term by term), over a chain of n = K + slabs + T + 4 roundings:
# K = the contraction length of one transform point, T = the sum over the six 1-D transform passes of 2 r - 1, r = the most
# non-zeros in a row of that pass's matrix (r multiplies and r - 1 adds can each round once).  The VALUE stays the direct oracle's.
# For a weight gradient the roles turn: dW = Gt [ sum_tiles (A dY At) (.) (Bt X B) ] G, contracted over the tiles.
_h = 0.5
WINO = {            # name -> (Bt, G, At)
    "F23": (np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64),
            np.array([[1, 0, 0], [_h, _h, _h], [_h, -_h, _h], [0, 0, 1]], np.float64),
            np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)),
    "F22": (np.array([[1, -1, 0], [0, 1, 0], [0, -1, 1]], np.float64),
            np.array([[1, 0], [1, 1], [0, 1]], np.float64),
            np.array([[1, 1, 0], [0, 1, 1]], np.float64)),
    "F43": (np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                      [0, 4, 0, -5, 0, 1]], np.float64),
            np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6],
                      [0, 0, 1]], np.float64),
            np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)),
}
WINO_SLABS_CONV, WINO_SLABS_WGRAD = 16, 512        # wino_plan / launch_wino22: at most 16 splits; the wgrad plans: at most 512
# the quantum of every intermediate on integer data: G of F(2x2,3x3) halves twice; F(2x2,2x2) stays in the integers
WINO_QUANTUM = {"F23": 0.25, "F22": 1.0}

WRes = namedtuple("WRes", Res._fields + ("alg", "vmax", "umax"))


def wino_T(alg, wgrad=False):
    """Roundings of the six 1-D transform passes (two per operand, two on the way out)."""
    Bt, G, At = WINO[alg]
    mats = (At.T, Bt, G.T) if wgrad else (Bt, G, At)
    return int(sum(2 * (2 * int((M != 0).sum(axis=1).max()) - 1) for M in mats))


def _cdiv(a, b):
    return -(-a // b)


def _tiles(xp, step, size, ty, tx):
    """[B][Hp][Wp][C] -> [B][ty][tx][C][size][size]: tile (i, j) starts at (i step, j step); zeros beyond the array."""
    B, Hp, Wp, C = xp.shape
    nh, nw = (ty - 1) * step + size, (tx - 1) * step + size
    xp = np.pad(xp, ((0, 0), (0, max(0, nh - Hp)), (0, max(0, nw - Wp)), (0, 0)))[:, :nh, :nw]
    v = np.lib.stride_tricks.sliding_window_view(xp, (size, size), axis=(1, 2))
    return v[:, ::step, ::step][:, :ty, :tx]


def wino_operands(xp, w, alg, OH, OW, absolute=False):
    """The transformed operands of wino_corr: Bt d B as [B][ty][tx][C][a][a] and G g Gt as [a][a][N][C]."""
    Bt, G, At = (np.abs(M) for M in WINO[alg]) if absolute else WINO[alg]
    m, a = At.shape[0], Bt.shape[0]
    assert w.shape[1] == w.shape[2] == G.shape[1] and w.shape[3] == xp.shape[3], (w.shape, xp.shape, alg)
    ty, tx = _cdiv(OH, m), _cdiv(OW, m)
    return Bt @ _tiles(f64(xp), m, a, ty, tx) @ Bt.T, np.einsum("au,nuvc,bv->abnc", G, f64(w), G)


def wino_woperands(xp, dy, alg, absolute=False):
    """The transformed operands of wino_wcorr: Bt X B as [B][ty][tx][C][a][a] and A dY At as [B][ty][tx][N][a][a]."""
    Bt, G, At = (np.abs(M) for M in WINO[alg]) if absolute else WINO[alg]
    m, a = At.shape[0], Bt.shape[0]
    ty, tx = _cdiv(dy.shape[1], m), _cdiv(dy.shape[2], m)
    return Bt @ _tiles(f64(xp), m, a, ty, tx) @ Bt.T, At.T @ _tiles(f64(dy), m, m, ty, tx) @ At


def wino_grid_ok(alg, mats, raw, transformed):
    """The condition of the rounded-operand reference.  `raw` = the arrays that enter the transforms `mats` (one matrix per
    array, applied from both sides), `transformed` = what comes out.  Every transformed operand is an integer multiple of the
    algorithm's quantum q, and max |raw| (largest absolute row sum of the matrix)^2, which bounds every partial sum of every
    evaluation order of the two passes, stays below 2^24 q: with coefficients +-1 and 1/2 any fp32 evaluation of the transform is
    then exact, and the bf16 operand is the rounding of an exact number."""
    q = WINO_QUANTUM[alg]
    for M, r, t in zip(mats, raw, transformed):
        n = t / q
        if not (np.array_equal(n, np.rint(n)) and float(np.abs(n).max(initial=0.0)) < EXACT_LIMIT):
            return False
        if float(np.abs(f64(r)).max(initial=0.0)) * float(np.abs(M).sum(axis=1).max()) ** 2 / q >= EXACT_LIMIT:
            return False
    return True


def _rounded(t, rnd):
    """A float64 array of fp32 numbers through `rnd` (fp32 -> fp32), as float64."""
    t32 = t.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t), "the transformed operand is not an fp32 number"
    return rnd(t32).astype(np.float64)


def wino_corr(xp, w, alg, OH, OW, absolute=False, rnd=None):
    """y[b][i][j][n] = sum_{u,v,c} xp[b][i + u][j + v][c] w[n][u][v][c] for i < OH, j < OW, evaluated in the Winograd domain of
    `alg` with tiles that start at (0, 0) -- or, `absolute`, S_w of that evaluation (the arguments are then magnitudes).
    `rnd`: the transformed operands pass through it (bf16_rne: what wino16.inc stores as V / U) before they are multiplied; the
    arguments are then the SIGNED data also where `absolute` -- the transforms do not round on the grid wino_grid_ok asserts, so
    S_w starts at the magnitudes of the rounded operands.
    Returns (y, max |Bt d B|, max |G g Gt|)."""
    Bt, G, At = WINO[alg]
    m, a = At.shape[0], Bt.shape[0]
    ty, tx = _cdiv(OH, m), _cdiv(OW, m)
    V, Uw = wino_operands(xp, w, alg, OH, OW, absolute and rnd is None)     # [B][ty][tx][C][a][a], [a][a][N][C]
    if rnd is not None:
        assert wino_grid_ok(alg, (Bt, G), (xp, w), (V, Uw)), "rounded-operand reference off its grid"
        V, Uw = _rounded(V, rnd), _rounded(Uw, rnd)
    if absolute:
        V, Uw, At = np.abs(V), np.abs(Uw), np.abs(At)
    B, N = xp.shape[0], w.shape[0]
    M = np.empty((B, ty, tx, N, a, a))
    for i in range(a):
        for j in range(a):
            M[..., i, j] = V[..., i, j] @ Uw[i, j].T
    Y = At @ M @ At.T                                                       # [B][ty][tx][N][m][m]
    y = Y.transpose(0, 1, 4, 2, 5, 3).reshape(B, ty * m, tx * m, N)[:, :OH, :OW]
    return y, float(np.abs(V).max()), float(np.abs(Uw).max())


def wino_wcorr(xp, dy, alg, absolute=False, rnd=None):
    """dw[n][u][v][c] = sum_{b,i,j} dy[b][i][j][n] xp[b][i + u][j + v][c] in the Winograd domain of `alg` contracted over the tiles
    of dy (they start at (0, 0)) -- or S_w of it.  `rnd`: as in wino_corr, applied to Bt X B and A dY At.
    Returns (dw, max |Bt X B|, max |A dY At|, number of tiles)."""
    Bt, G, At = WINO[alg]
    m, a = At.shape[0], Bt.shape[0]
    B, OH, OW, N = dy.shape
    ty, tx = _cdiv(OH, m), _cdiv(OW, m)
    V, Yt = wino_woperands(xp, dy, alg, absolute and rnd is None)           # [B][ty][tx][C][a][a], [B][ty][tx][N][a][a]
    if rnd is not None:
        assert wino_grid_ok(alg, (Bt, At.T), (xp, dy), (V, Yt)), "rounded-operand reference off its grid"
        V, Yt = _rounded(V, rnd), _rounded(Yt, rnd)
    if absolute:
        V, Yt, G = np.abs(V), np.abs(Yt), np.abs(G)
    C = xp.shape[3]
    M = np.empty((a, a, N, C))
    for i in range(a):
        for j in range(a):
            M[i, j] = Yt[..., i, j].reshape(-1, N).T @ V[..., i, j].reshape(-1, C)
    dw = np.einsum("ua,abnc,bv->nuvc", G.T, M, G)
    return dw, float(np.abs(V).max()), float(np.abs(Yt).max()), B * ty * tx


# the two regroupings that put the stride-2 layers on stride-1 Winograd kernels
def s2d(x):
    """x2[b][yy][xx][(dy, dx, c)] = x[b][2 yy + dy][2 xx + dx][c]  (5x5 / stride 2 / pad 2 as 3x3 / stride 1 / pad 1 over 4 C)."""
    B, H, W, C = x.shape
    return x.reshape(B, H // 2, 2, W // 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, H // 2, W // 2, 4 * C)


def d2s(x2):
    B, H2, W2, C4 = x2.shape
    C = C4 // 4
    return x2.reshape(B, H2, W2, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * H2, 2 * W2, C)


def w_regroup(w, t):
    """w2[co][ty][tx][(dy, dx, c)] = w[co][2 ty + dy][2 tx + dx][c] with t x t taps (0 where the tap does not exist)."""
    Cout, k, _, C = w.shape
    wp = np.zeros((Cout, 2 * t, 2 * t, C), w.dtype)
    wp[:, :k, :k] = w
    return wp.reshape(Cout, t, 2, t, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(Cout, t, t, 4 * C)


def w_ungroup(w2, k):
    Cout, t, _, C4 = w2.shape
    C = C4 // 4
    return w2.reshape(Cout, t, t, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(Cout, 2 * t, 2 * t, C)[:, :k, :k]


def s2d_shifted(x):
    """x2[b][yy][xx][(dy, dx, c)] = x[b][2 yy + dy - 1][2 xx + dx - 1][c], yy <= H / 2 (4x4 / stride 2 / pad 1 as 2x2 valid)."""
    return s2d(_pad(x, 1))


def _flip(w):
    """The correlation weights of a stride-1 dgrad: w'[ci][u][v][co] = w[co][k - 1 - u][k - 1 - v][ci]."""
    return w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0)


def wino_kind(k, s, p):
    return {(3, 1): "s1", (5, 2): "s2d", (4, 2): "w22"}[(k, s)]


# The three functions below reduce every Winograd route to stride-1 problems of wino_corr / wino_wcorr.  `corr` / `wcorr`: another
# evaluation of those problems with the same signature (tests/test_wino_oracle_cpu.py: an fp32 emulation) in place of the oracle's.
def _wino_fwd_corr(xin, w, k, s, p, alg, absolute, corr=None):
    corr = corr or (lambda *a: wino_corr(*a, absolute))
    B, H, W, Cin = xin.shape
    Ho, Wo = out_size(H, k, s, p), out_size(W, k, s, p)
    kind = wino_kind(k, s, p)
    if kind == "s1":
        return corr(_pad(xin, p), w, alg, Ho, Wo), Cin
    if kind == "s2d":
        assert p == 2 and alg == "F23"
        return corr(_pad(s2d(xin), 1), w_regroup(w, 3), alg, Ho, Wo), 4 * Cin
    assert p == 1 and alg == "F22"
    return corr(s2d_shifted(xin), w_regroup(w, 2), alg, Ho, Wo), 4 * Cin


def _wino_dgrad_corr(dy, w, x_shape, k, s, p, alg, absolute, corr=None):
    corr = corr or (lambda *a: wino_corr(*a, absolute))
    B, H, W, Cin = x_shape
    Cout = w.shape[0]
    kind = wino_kind(k, s, p)
    if kind == "s1":
        return corr(_pad(dy, k - 1 - p), _flip(w), alg, H, W)
    if kind == "s2d":
        y2, vm, um = corr(_pad(dy, 1), _flip(w_regroup(w, 3)), alg, H // 2, W // 2)
        return d2s(y2), vm, um
    # four parity classes: dx[2 y' + 1 - dy][2 x' + 1 - dx][c] = sum w[co][2 ty + dy][2 tx + dx][c] g[y' + 1 - dy - ty][x' + 1 - dx - tx][co]
    gp = _pad(dy, 1)
    Ho, Wo = dy.shape[1], dy.shape[2]
    out, vm, um = np.zeros((B, H, W, Cin), dy.dtype), 0.0, 0.0
    for cy in range(2):
        for cx in range(2):
            wc = w[:, cy::2, cx::2, :][:, ::-1, ::-1, :].transpose(3, 1, 2, 0)          # [c][u = 1 - ty][v = 1 - tx][co]
            yc, v1, u1 = corr(gp[:, 1 - cy:, 1 - cx:], wc, alg, Ho, Wo)
            out[:, 1 - cy::2, 1 - cx::2] = yc
            vm, um = max(vm, v1), max(um, u1)
    return out, vm, um


def wino_fwd(x, w, k, s, p, alg, mask=None, bias=None, ratio=None, act_kind=ACT_NONE, slope=0.0):
    d = conv_fwd(x, w, k, s, p, mask, bias, ratio, act_kind, slope)
    xabs = _source(x, mask, None)[1]
    (S, vm, um), K = _wino_fwd_corr(xabs, np.abs(f64(w)), k, s, p, alg, True)
    if bias is not None:
        S = S + np.abs(f64(bias))
    return WRes(d.val, S, np.full(S.shape, float(K + wino_T(alg))), d.scale, d.base, False, alg, vm, um)


def wino_dgrad(dy, w, x_shape, k, s, p, alg, mask=None, gate=None, gate_act=ACT_RELU, gate_slope=0.0, base=None):
    d = conv_dgrad(dy, w, x_shape, k, s, p, mask, gate, gate_act, gate_slope, base)
    S, vm, um = _wino_dgrad_corr(np.abs(f64(dy)), np.abs(f64(w)), x_shape, k, s, p, alg, True)
    return WRes(d.val, S, np.full(S.shape, float(np.shape(w)[0] + wino_T(alg))), d.scale, d.base, False, alg, vm, um)


def _wino_wgrad_corr(xin, dy, k, s, p, alg, absolute, wcorr=None):
    wcorr = wcorr or (lambda *a: wino_wcorr(*a, absolute))
    kind = wino_kind(k, s, p)
    if kind == "s1":
        return wcorr(_pad(xin, p), dy, alg)
    if kind == "s2d":
        dw2, vm, ym, nt = wcorr(_pad(s2d(xin), 1), dy, alg)
        return w_ungroup(dw2, 5), vm, ym, nt
    dw2, vm, ym, nt = wcorr(s2d_shifted(xin), dy, alg)
    return w_ungroup(dw2, 4), vm, ym, nt


def wino_wgrad(x, dy, k, s, p, alg):
    """(dW, db): dW through the Winograd weight gradient of `alg` (F23: F(3x3,2x2); F22: F(2x2,2x2)), db the direct column sum."""
    rw, rb = conv_wgrad(x, dy, k, s, p)
    S, vm, ym, ntiles = _wino_wgrad_corr(np.abs(f64(x)), np.abs(f64(dy)), k, s, p, alg, True)
    K = np.full(S.shape, float(ntiles + wino_T(alg, wgrad=True)))
    return WRes(rw.val, S, K, rw.scale, rw.base, False, alg, vm, ym), rb


# ---- the bf16 Winograd kernels (wino16.inc): the reference that rounds where the kernel rounds ------------------------------------------
# Both transforms are fp32, the transformed operands are rounded to bf16 once (at the V / U store; A dY At and Bt X B in the weight
# gradient), the products run on a bf16 MFMA with fp32 accumulation, the output transform is fp32.  On data for which the
# transforms are exact in fp32 (wino_grid_ok, asserted by wino_corr / wino_wcorr) the bf16 operands are fully determined -- RNE of
# exact numbers -- and what is left to round is the contraction and the output transform:
#     value = At [ sum_c rnd(G g Gt) (.) rnd(Bt d B) ] A         S = |At| [ sum_c |rnd(G g Gt)| (.) |rnd(Bt d B)| ] |A|
# with n = K + slabs + T + 4 as for the fp32 kernels (T keeps the roundings of the operand transforms, which cannot happen here: a
# safe over-count).  Bias, ratio, mask, gate, activation and base follow as in conv_fwd / conv_dgrad; db stays the fp32 column
# sum of the unrounded dy.
def wino_fwd_rounded(x, w, k, s, p, alg, mask=None, bias=None, ratio=None, act_kind=ACT_NONE, slope=0.0, rnd=bf16_rne):
    xin = _source(x, mask, None)[0]
    w = f64(w)
    (z, vm, um), K = _wino_fwd_corr(xin, w, k, s, p, alg, False, lambda *a: wino_corr(*a, rnd=rnd))
    S = _wino_fwd_corr(xin, w, k, s, p, alg, True, lambda *a: wino_corr(*a, absolute=True, rnd=rnd))[0][0]
    if bias is not None:
        z, S = z + f64(bias), S + np.abs(f64(bias))
    scale = np.ones(z.shape[:3] + (1,))
    if ratio is not None:
        z, scale = z * f64(ratio)[..., None], np.abs(f64(ratio))[..., None]
    return WRes(act(z, act_kind, slope), S, np.full(S.shape, float(K + wino_T(alg))), np.broadcast_to(scale, S.shape),
                np.zeros_like(S), False, alg, vm, um)


def wino_dgrad_rounded(dy, w, x_shape, k, s, p, alg, mask=None, gate=None, gate_act=ACT_RELU, gate_slope=0.0, base=None,
                       rnd=bf16_rne):
    dy, w = f64(dy), f64(w)
    dx, vm, um = _wino_dgrad_corr(dy, w, x_shape, k, s, p, alg, False, lambda *a: wino_corr(*a, rnd=rnd))
    S = _wino_dgrad_corr(dy, w, x_shape, k, s, p, alg, True, lambda *a: wino_corr(*a, absolute=True, rnd=rnd))[0]
    scale = np.ones(dx.shape)
    if mask is not None:
        scale = scale * f64(mask)[..., None]
    if gate is not None:
        scale = scale * act_grad(f64(gate), gate_act, gate_slope)
    dx, b0 = dx * scale, np.zeros_like(dx)
    if base is not None:
        dx, b0 = dx + f64(base), np.abs(f64(base))
    return WRes(dx, S, np.full(S.shape, float(w.shape[0] + wino_T(alg))), np.abs(scale), b0, False, alg, vm, um)


def wino_wgrad_rounded(x, dy, k, s, p, alg, rnd=bf16_rne):
    """(dW, db): dW from the rounded A dY At and Bt X B, db the direct column sum of the dy as given."""
    x, dy = f64(x), f64(dy)
    dw, vm, ym, ntiles = _wino_wgrad_corr(x, dy, k, s, p, alg, False, lambda *a: wino_wcorr(*a, rnd=rnd))
    S = _wino_wgrad_corr(x, dy, k, s, p, alg, True, lambda *a: wino_wcorr(*a, absolute=True, rnd=rnd))[0]
    K = np.full(S.shape, float(ntiles + wino_T(alg, wgrad=True)))
    return WRes(dw, S, K, np.ones_like(S), np.zeros_like(S), False, alg, vm, ym), conv_wgrad(x, dy, k, s, p)[1]


def wino_exact_ok(r, bf16=False):
    """Integer data: every intermediate is a multiple of the algorithm's quantum q and bounded by S_w, so with max S_w / q < 2^24
    every partial sum of every order is an fp32 number.  bf16 operands: the transformed operands (bounded here by their
    absolute-value twins, which is the stronger demand) must also be bf16 numbers: |V| <= 256 and |U| / q <= 256."""
    q = WINO_QUANTUM[r.alg]
    ok = float((r.S * np.maximum(r.scale, 1.0) + r.base).max()) / q < EXACT_LIMIT
    return ok and (not bf16 or (r.vmax <= 256.0 and r.umax / q <= 256.0))
