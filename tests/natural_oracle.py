"""numpy oracle of the natural-neighbour (discrete Sibson) void fill (csrc/natural.hip, mvp_gan/src/natural.py, DESIGN.md section
8ai).  Written from the definition, not from the kernel:

  d2(q), idx(q)  idw_oracle.nearest of the known map, uncapped (brute force over all seeds; its tie rule);
  nn(q)          idw_oracle.gather_fill: z(q) on a known pixel, z[idx(q)] on a void one, NaN without any known pixel;
  c(q)           min(d2(q), radius^2), radius an integer in [1, 32];
  out(p)         for a void p: (float32)(sum nn(q) / n(p)) over the q with |p - q|^2 < c(q) (integers, strictly), the sum in
                 float64 from 0.0 in row-major order of q, n(p) their number; NaN where idx(p) < 0 or, with lim2 > 0,
                 d2(p) > lim2 (the limit masks the output only); known pixels come back bit for bit;
  support(p)     n(p), 0 on known pixels.

natural() walks the window offsets (dy, dx) in row-major order over whole planes, every step one elementwise float64 addition;
natural_brute() is the definition as a per-pixel double loop over the whole raster, for tiny rasters."""
import math

import numpy as np

from tests import idw_oracle as IO

MAX_RADIUS = 32


def _setup(z, known, radius):
    z = np.asarray(z, np.float32)
    kn = np.asarray(known) != 0
    assert z.shape == kn.shape and z.ndim == 2
    assert isinstance(radius, (int, np.integer)) and not isinstance(radius, bool) and 1 <= radius <= MAX_RADIUS
    d2, idx = IO.nearest(kn)
    nn, _ = IO.gather_fill(z, kn, idx)
    c = np.minimum(d2.astype(np.int64), int(radius) * int(radius))
    return z, kn, d2, idx, nn, c


def _finish(z, kn, d2, idx, s, n, lo, hi, lim2):
    left = ~kn & (idx < 0)
    if lim2 > 0:
        left |= ~kn & (d2.astype(np.int64) > lim2)
    fill = ~kn & ~left
    out = np.where(kn, z, np.float32(np.nan)).astype(np.float32)
    out[fill] = (s[fill] / n[fill].astype(np.float64)).astype(np.float32)
    lo, hi = lo.astype(np.float32), hi.astype(np.float32)
    lo[~fill], hi[~fill] = np.nan, np.nan
    support = np.where(kn, 0, n).astype(np.int32)
    return out, support, [int(fill.sum()), int(left.sum())], lo, hi


def natural(z, known, radius, lim2=0):
    """-> (out float32 [H][W], support int32 [H][W], counts [filled, left NaN], lo, hi float32 [H][W]: the smallest and the
    largest contributing nn of every filled pixel, NaN elsewhere).  Vectorised over the window offsets in row-major order; the
    window R = min(radius - 1, ceil(sqrt(max c))) holds every contributor."""
    z, kn, d2, idx, nn, c = _setup(z, known, radius)
    H, W = kn.shape
    R = min(int(radius) - 1, math.isqrt(int(c.max()) - 1) + 1 if c.max() > 0 else 0)
    cp = np.zeros((H + 2 * R, W + 2 * R), np.int64)
    cp[R:R + H, R:R + W] = c
    vp = np.zeros((H + 2 * R, W + 2 * R), np.float32)
    vp[R:R + H, R:R + W] = nn
    s, n = np.zeros((H, W), np.float64), np.zeros((H, W), np.int64)
    lo, hi = np.full((H, W), np.inf, np.float32), np.full((H, W), -np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                cq, vq = cp[R + dy:R + dy + H, R + dx:R + dx + W], vp[R + dy:R + dy + H, R + dx:R + dx + W]
                ok = ~kn & (dy * dy + dx * dx < cq)
                if not ok.any():
                    continue
                s = np.where(ok, s + vq.astype(np.float64), s)
                n += ok
                lo, hi = np.where(ok, np.minimum(lo, vq), lo), np.where(ok, np.maximum(hi, vq), hi)
    return _finish(z, kn, d2, idx, s, n, lo, hi, lim2)


def natural_brute(z, known, radius, lim2=0):
    """The same five results by the definition itself: for every void pixel p a loop over every raster pixel q in row-major
    order."""
    z, kn, d2, idx, nn, c = _setup(z, known, radius)
    H, W = kn.shape
    s, n = np.zeros((H, W), np.float64), np.zeros((H, W), np.int64)
    lo, hi = np.full((H, W), np.inf, np.float32), np.full((H, W), -np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        for py in range(H):
            for px in range(W):
                if kn[py, px]:
                    continue
                acc, cnt = np.float64(0.0), 0
                for qy in range(H):
                    for qx in range(W):
                        if (py - qy) ** 2 + (px - qx) ** 2 < int(c[qy, qx]):
                            acc = acc + np.float64(nn[qy, qx])
                            cnt += 1
                            lo[py, px], hi[py, px] = min(lo[py, px], nn[qy, qx]), max(hi[py, px], nn[qy, qx])
                s[py, px], n[py, px] = acc, cnt
    return _finish(z, kn, d2, idx, s, n, lo, hi, lim2)
