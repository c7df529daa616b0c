"""numpy fp64 oracle of the BatchNorm family of csrc/pointwise.hip (tg_bn_stats / tg_bn_fwd / tg_bn_act_fwd / tg_bn_act_bwd /
tg_bn_act_bwd_conv1, the grouped forms and the running-statistics updates).  Plain restatements of the formulas, independent of
the package: nothing here imports tg_hip or torch.  Inputs are converted to float64 on entry, so a test evaluates the oracle on
the very fp32 values the kernel reads.  Matrices are [rows][C]; per-channel vectors are [C]."""
import numpy as np

from tests.pointwise_oracle import ACT_LEAKY, ACT_NONE, ACT_RELU, err, f64  # noqa: F401  (err: the relative figure tests print)

U = 2.0 ** -24          # unit roundoff of fp32


def ulp32(x):
    """Spacing of fp32 at |x| (of the rounded value), as float64."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- statistics -------------------------------------------------------------------------------------------------------------
def stats(y, eps):
    """-> (mean, biased var, rstd = 1 / sqrt(var + eps)) per channel."""
    y = f64(y)
    mean = y.mean(axis=0)
    var = ((y - mean) ** 2).mean(axis=0)
    return mean, var, 1.0 / np.sqrt(var + eps)


def running(rm, rv, mean, var, n, momentum):
    """One training-mode update of the running statistics; the running variance takes the unbiased estimate var * n / (n - 1)."""
    rm, rv, mean, var = f64(rm), f64(rv), f64(mean), f64(var)
    return (1.0 - momentum) * rm + momentum * mean, (1.0 - momentum) * rv + momentum * var * (n / (n - 1.0))


def var_of_rstd(rstd, eps):
    """The biased variance a saved rstd stands for (what tg_bn_running_update is given): max(1 / rstd^2 - eps, 0)."""
    r = f64(rstd)
    return np.maximum(1.0 / (r * r) - eps, 0.0)


# ---- forward ----------------------------------------------------------------------------------------------------------------
def act_fwd(z, act, slope):
    if act == ACT_NONE:
        return z
    return np.where(z > 0, z, 0.0 if act == ACT_RELU else z * slope)


def act_grad(z, act, slope):
    if act == ACT_NONE:
        return np.ones_like(z)
    return np.where(z > 0, 1.0, 0.0 if act == ACT_RELU else slope)


def apply(y, mean, rstd, gamma, beta, act, slope=0.0):
    xh = (f64(y) - f64(mean)) * f64(rstd)
    return act_fwd(xh * f64(gamma) + f64(beta), act, slope)


# ---- backward ---------------------------------------------------------------------------------------------------------------
def bwd(dout, y, mean, rstd, gamma, beta, act, slope=0.0, ratio=None):
    """-> (dy, dgamma, dbeta, dbias, q [5][C]).
    g = dout * act'(z), z = xh * gamma + beta, act' from z > 0; dbeta = sum g, dgamma = sum g * xh;
    dy = gamma * rstd * (g - dbeta / n - xh * dgamma / n) * ratio; dbias = sum_rows dy.
    q = (sum g, sum g xh, sum ratio g, sum ratio xh, sum ratio).  dbias is evaluated from them in closed form,
    gamma rstd (q2 - q0 q4 / n - q1 q3 / n): the same number as the sum over rows of dy, without that sum's own rounding (with the
    dyadic inputs of tests/bn_cases.py the five sums are exact, a sum of thousands of fp64 dy is not)."""
    dout, y, mean, rstd, gamma, beta = f64(dout), f64(y), f64(mean), f64(rstd), f64(gamma), f64(beta)
    n = float(y.shape[0])
    rr = np.ones(y.shape[0]) if ratio is None else f64(ratio).reshape(-1)
    rr = rr[:, None]
    xh = (y - mean) * rstd
    g = dout * act_grad(xh * gamma + beta, act, slope)
    q = np.stack([g.sum(0), (g * xh).sum(0), (rr * g).sum(0), (rr * xh).sum(0), np.broadcast_to(rr, y.shape).sum(0)])
    dbeta, dgamma = q[0], q[1]
    dy = gamma * rstd * (g - dbeta / n - xh * dgamma / n) * rr
    dbias = gamma * rstd * (q[2] - q[0] * q[4] / n - q[1] * q[3] / n)
    return dy, dgamma, dbeta, dbias, q


def bwd_terms(dout, y, mean, rstd, gamma, beta, act, slope=0.0, ratio=None):
    """|g|, |xh| of bwd, for the per-element error bound of dy."""
    dout, y = f64(dout), f64(y)
    xh = (y - f64(mean)) * f64(rstd)
    return np.abs(dout * act_grad(xh * f64(gamma) + f64(beta), act, slope)), np.abs(xh)


def conv1_dgrad(dz, w):
    """Input gradient of a C -> 1 channel 3x3 / stride 1 / pad 1 convolution: dz [B][H][W], w [3][3][C] ->
    dout[b][y][x][c] = sum_{ky,kx} dz[b][y + 1 - ky][x + 1 - kx] * w[ky][kx][c], zero outside the image."""
    dz, w = f64(dz), f64(w)
    B, H, W = dz.shape
    p = np.zeros((B, H + 2, W + 2))
    p[:, 1:-1, 1:-1] = dz
    out = np.zeros((B, H, W, w.shape[2]))
    for ky in range(3):
        for kx in range(3):
            # dz[y + 1 - ky] = p[y + 2 - ky]
            out += p[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W, None] * w[ky, kx]
    return out


# ---- grouped forms: `groups` passes stacked along the rows, statistics per pass --------------------------------------------
def stats_grouped(y, groups, eps):
    """-> (mean, var, rstd), each [groups][C]."""
    y = f64(y)
    rows_g = y.shape[0] // groups
    res = [stats(y[g * rows_g:(g + 1) * rows_g], eps) for g in range(groups)]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


def apply_grouped(y, groups, mean, rstd, gamma, beta, act, slope=0.0):
    y = f64(y)
    rows_g = y.shape[0] // groups
    return np.concatenate([apply(y[g * rows_g:(g + 1) * rows_g], mean[g], rstd[g], gamma, beta, act, slope) for g in range(groups)])


def bwd_grouped(dout, y, groups, mean, rstd, gamma, beta, act, slope=0.0):
    """-> (dy, dgamma, dbeta, dbias, per-group list of bwd results).  The parameter gradients of the passes are rounded to fp32
    and summed in pass order in fp32, as bn_bwd_final_grouped_kernel documents (what accumulating separate calls gave)."""
    dout, y = f64(dout), f64(y)
    rows_g = y.shape[0] // groups
    per = [bwd(dout[g * rows_g:(g + 1) * rows_g], y[g * rows_g:(g + 1) * rows_g], mean[g], rstd[g], gamma, beta, act, slope)
           for g in range(groups)]
    acc = [None, None, None]
    for r in per:
        for i, v in enumerate((r[1], r[2], r[3])):
            v32 = v.astype(np.float32)
            acc[i] = v32 if acc[i] is None else (v32 + acc[i]).astype(np.float32)
    return np.concatenate([r[0] for r in per]), acc[0], acc[1], acc[2], per


def running_multi(rm, rv, mean, var, n, momentum, order):
    """Updates of passes `order` (indices into mean / var [groups][C]) one after the other; the buffers are fp32, so every
    update rounds to fp32 before the next one reads it."""
    rm, rv = np.asarray(rm, dtype=np.float32), np.asarray(rv, dtype=np.float32)
    for g in order:
        a, b = running(rm, rv, mean[g], var[g], n, momentum)
        rm, rv = a.astype(np.float32), b.astype(np.float32)
    return rm, rv
