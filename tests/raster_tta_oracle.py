"""numpy mirrors of the test-time augmentation kernels (csrc/raster.hip: tg_raster_gather_ops, tg_raster_tta_reduce,
tg_raster_blend_tta), built on tests/raster_oracle.py: the eight transforms and their inverses, the member reduction in float32
in the kernel's order (it must match bit for bit), the blend with its spread in float64."""
import numpy as np

from tests import raster_oracle as RO

OPS = (0, 1, 2, 3, 4, 5, 6, 7)


def transform(frame, op):
    """Member frame of a window frame [..., wh, ww]: member pixel (i, j) reads window pixel (a, b) = op & 4 ? (j, i) : (i, j),
    then a = wh-1-a if op & 2 and b = ww-1-b if op & 1: the flips first, then the transposition."""
    y = np.asarray(frame)
    if op & 2:
        y = y[..., ::-1, :]
    if op & 1:
        y = y[..., :, ::-1]
    if op & 4:
        y = np.swapaxes(y, -1, -2)
    return np.ascontiguousarray(y)


def inverse(frame, op):
    """Window frame of a member frame: transform undone (the transposition first, then the flips, each its own inverse)."""
    y = np.asarray(frame)
    if op & 4:
        y = np.swapaxes(y, -1, -2)
    if op & 2:
        y = y[..., ::-1, :]
    if op & 1:
        y = y[..., :, ::-1]
    return np.ascontiguousarray(y)


def reduce(gout, ops):
    """gout float32 [n][T][wh][ww], member t under ops[t] -> (mean, var) float32 [n][wh][ww] in the window frame:
    mean = (o_0 + ... + o_{T-1}) * (1 / T), var = sum_t (o_t - mean)^2 / (T - 1), every operation rounded to float32, added in
    member order."""
    gout = np.asarray(gout, np.float32)
    T = gout.shape[1]
    assert T == len(ops) and T in (2, 4, 8)
    o = [inverse(gout[:, t], ops[t]) for t in range(T)]
    with np.errstate(invalid="ignore", over="ignore"):
        s = o[0]
        for t in range(1, T):
            s = (s + o[t]).astype(np.float32)
        mean = (s * np.float32(1.0 / T)).astype(np.float32)
        e = (o[0] - mean).astype(np.float32)
        ss = (e * e).astype(np.float32)
        for t in range(1, T):
            e = (o[t] - mean).astype(np.float32)
            ss = (ss + (e * e).astype(np.float32)).astype(np.float32)
        var = (ss / np.float32(T - 1)).astype(np.float32)
    return mean, var


def blend_tta(z, plan, lo, hi, run_of_window, wmean, wvar, mask=None, nodata=None):
    """float64: RO.blend of the means, and per hole spread = sqrt(sum_j w_j (var_j d_j^2 + (dn_j - out)^2) / sum_j w_j) over the
    running covering windows (d_j = hi_j - lo_j, dn_j = lo_j + mean_j d_j); 0 at known pixels, NaN where none covers.
    -> (raster, spread, unfilled count)."""
    out, unfilled = RO.blend(z, plan, lo, hi, run_of_window, wmean, mask, nodata)
    k = RO.known(z, mask, nodata)
    acc = np.zeros(z.shape)
    den = np.zeros(z.shape)
    for j, (y0, x0) in enumerate(RO.windows(plan)):
        r = run_of_window[j]
        if r < 0:
            continue
        wy = RO.ramp(plan.wh, plan.overlap, y0 == 0, y0 + plan.wh == plan.H)
        wx = RO.ramp(plan.ww, plan.overlap, x0 == 0, x0 + plan.ww == plan.W)
        w = wy[:, None] * wx[None, :]
        l, h = float(lo[j]), float(hi[j])
        d = h - l
        sl = (slice(y0, y0 + plan.wh), slice(x0, x0 + plan.ww))
        with np.errstate(invalid="ignore"):
            dev = l + wmean[r].astype(np.float64) * d - out[sl]
        acc[sl] += w * (wvar[r].astype(np.float64) * d * d + dev * dev)
        den[sl] += w
    with np.errstate(invalid="ignore", divide="ignore"):
        spread = np.where(den > 0, np.sqrt(acc / den), np.nan)
    return out, np.where(k, 0.0, spread), unfilled
