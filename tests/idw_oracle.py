"""numpy oracle of the feature transform and of the directional inverse-distance, nearest-neighbour and smoothing fills
(csrc/edt.hip, csrc/idw.hip, mvp_gan/src/interpolate.py).  Written from the definitions, not from the
kernels: the rays are followed step by step along each direction, the nearest seed is a brute-force minimum over all seeds in
int64, and every floating-point step is one elementwise np.float64 operation (numpy does not fuse a multiply into an add)."""
import math

import numpy as np

FAR = 0x7fffffff
DIRS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))      # N, NE, E, SE, S, SW, W, NW
SCALE = (1, 2, 1, 2, 1, 2, 1, 2)                                                  # s_j: squared length of one step


def nearest(seed, cap2=0, chunk=4096):
    """-> (d2 int32 [H][W], idx int32 [H][W]): the squared distance to the nearest nonzero pixel of seed, min'ed with cap2
    (> 0), FAR without a seed and a cap; idx = y * W + x of the nearest seed, the smallest row and then the smallest column
    among those at the smallest distance, -1 where d2 is FAR or d2 >= cap2.  Brute force over all seeds."""
    s = np.asarray(seed) != 0
    H, W = s.shape
    ys, xs = np.nonzero(s)                                  # row-major: sorted by (row, column)
    d2 = np.full(H * W, FAR, np.int64)
    idx = np.full(H * W, -1, np.int64)
    if ys.size:
        py, px = np.divmod(np.arange(H * W, dtype=np.int64), W)
        for a in range(0, H * W, chunk):
            d = (py[a:a + chunk, None] - ys[None, :]) ** 2 + (px[a:a + chunk, None] - xs[None, :]) ** 2
            j = d.argmin(axis=1)                            # the first minimum: the lexicographically smallest (row, column)
            d2[a:a + chunk] = d[np.arange(len(j)), j]
            idx[a:a + chunk] = ys[j] * W + xs[j]
    if cap2 > 0:
        idx[d2 >= cap2] = -1
        d2 = np.minimum(d2, cap2)
    return d2.reshape(H, W).astype(np.int32), idx.reshape(H, W).astype(np.int32)


def ray_hits(known, lim2=0):
    """uint16 [8][H][W]: per direction the number of steps to the first known pixel, 0 without one inside the raster or with
    k^2 s > lim2 (lim2 <= 0: no limit); 0 on known pixels.  One explicit sweep along each direction, against it: with q = p + d,
    k[p] = 1 where q is known, k[q] + 1 where q is unknown and has a hit, 0 where q is outside the raster or has none."""
    kn = np.asarray(known) != 0
    H, W = kn.shape
    hits = np.zeros((8, H, W), np.int64)
    for j, (dy, dx) in enumerate(DIRS):
        k = hits[j]
        if dy:                                                  # row by row, starting at the edge the rays run into
            for y in (range(1, H) if dy < 0 else range(H - 2, -1, -1)):
                x0, x1 = max(0, -dx), W - max(0, dx)            # the columns whose q = (y + dy, x + dx) is inside
                qk, qh = kn[y + dy, x0 + dx:x1 + dx], k[y + dy, x0 + dx:x1 + dx]
                k[y, x0:x1] = np.where(qk, 1, np.where(qh > 0, qh + 1, 0))
        else:                                                   # column by column
            for x in (range(1, W) if dx < 0 else range(W - 2, -1, -1)):
                qk, qh = kn[:, x + dx], k[:, x + dx]
                k[:, x] = np.where(qk, 1, np.where(qh > 0, qh + 1, 0))
        k[kn] = 0
        if lim2 > 0:
            k[k * k * SCALE[j] > lim2] = 0
    return hits.astype(np.uint16)


def weight(n, power):
    """fp64 [..]: the weight of a hit at squared distance n (an integer array)."""
    n = np.asarray(n).astype(np.float64)
    if power == 2:
        return np.float64(1.0) / n
    if power == 1:
        return np.float64(1.0) / np.sqrt(n)
    return np.power(n, np.float64(-float(power) / 2.0))


def rayfill(z, known, lim2=0, power=2.0, d2=None, idx=None, hits=None):
    """-> (out float32 [H][W], counts [by rays, by nearest, left NaN], lo, hi float32 [H][W]: the smallest and largest
    contributing height of every pixel filled by rays, NaN elsewhere).  Elementwise numpy: a product and a sum are two
    separately rounded operations."""
    z = np.asarray(z, np.float32)
    kn = np.asarray(known) != 0
    H, W = kn.shape
    hits = ray_hits(kn, lim2) if hits is None else hits
    y, x = np.mgrid[0:H, 0:W]
    num, den = np.zeros((H, W), np.float64), np.zeros((H, W), np.float64)
    lo, hi = np.full((H, W), np.inf, np.float32), np.full((H, W), -np.inf, np.float32)
    for j, (dy, dx) in enumerate(DIRS):
        k = hits[j].astype(np.int64)
        m = k > 0
        w = weight((k * k * SCALE[j])[m], power)
        zj = z[(y + k * dy)[m], (x + k * dx)[m]]
        num[m] = num[m] + w * zj.astype(np.float64)
        den[m] = den[m] + w
        lo[m], hi[m] = np.minimum(lo[m], zj), np.maximum(hi[m], zj)
    rays = ~kn & (hits != 0).any(axis=0)
    out = np.where(kn, z, np.float32(np.nan)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[rays] = (num[rays] / den[rays]).astype(np.float32)
    near = np.zeros((H, W), bool)
    if idx is not None:
        near = ~kn & ~rays & (idx >= 0)
        if lim2 > 0:
            near &= (d2 >= 0) & (d2 <= lim2)
        out[near] = z.ravel()[idx[near]]
    lo[~rays], hi[~rays] = np.nan, np.nan
    return out, [int(rays.sum()), int(near.sum()), int((~kn & ~rays & ~near).sum())], lo, hi


def gather_fill(z, known, idx):
    """-> (out float32 [H][W], [filled, left NaN])."""
    z = np.asarray(z, np.float32)
    kn = np.asarray(known) != 0
    ok = ~kn & (idx >= 0)
    out = np.where(kn, z, np.float32(np.nan)).astype(np.float32)
    out[ok] = z.ravel()[idx[ok]]
    return out, [int(ok.sum()), int((~kn & (idx < 0)).sum())]


def smooth(a, known, steps=1):
    """`steps` Jacobi steps: an unknown, non-NaN pixel becomes the fp64 sum in row-major order of the non-NaN pixels of its
    clipped 3x3 neighbourhood over their count, rounded to float32 once; known and NaN pixels are copied."""
    a = np.asarray(a, np.float32).copy()
    kn = np.asarray(known) != 0
    H, W = a.shape
    for _ in range(steps):
        pad = np.full((H + 2, W + 2), np.nan, np.float32)
        pad[1:-1, 1:-1] = a
        s, n = np.zeros((H, W), np.float64), np.zeros((H, W), np.int64)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                v = pad[dy:dy + H, dx:dx + W]
                ok = ~np.isnan(v)
                s = np.where(ok, s + np.where(ok, v, 0).astype(np.float64), s)
                n += ok
        mv = ~kn & ~np.isnan(a)
        b = a.copy()
        b[mv] = (s[mv] / n[mv].astype(np.float64)).astype(np.float32)
        a = b
    return a


def ray_px2(max_distance, cellsize):
    """The largest integer n with cellsize * sqrt(n) <= max_distance in fp64, by bisection on that (monotone) predicate."""
    ok = lambda n: cellsize * math.sqrt(n) <= max_distance
    if not ok(0):
        return -1
    lo, hi = 0, 1                                           # ok(lo), and hi is doubled until it fails
    while ok(hi):
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo
