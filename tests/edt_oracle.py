"""numpy oracle of the exact Euclidean distance transform and the errors by depth (csrc/edt.hip, mvp_gan/src/distance.py,
DESIGN.md section 8r).  Written from the definitions, not from the kernels: the squared distance is a column scan followed by
a brute-force minimum over every column of the row, O(H W^2), in int64."""
import math

import numpy as np

FAR = 0x7fffffff
NONE = 1 << 40                      # no seed in the column: larger than any squared distance, small enough to add in int64


def column_distance(seed):
    """g int64 [H][W]: the vertical distance to the nearest seed of the same column, NONE where the column has none."""
    s = np.asarray(seed) != 0
    H, W = s.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(s, rows, -NONE), axis=0)                     # nearest seed row at or above
    nxt = np.minimum.accumulate(np.where(s, rows, NONE)[::-1], axis=0)[::-1]           # nearest seed row at or below
    return np.minimum(np.where(last < 0, NONE, rows - last), np.where(nxt >= NONE, NONE, nxt - rows))


def edt_d2(seed, cap2=0):
    """int32 [H][W]: min(exact squared Euclidean distance in pixels to the nearest nonzero pixel of seed, cap2); cap2 <= 0: no
    cap, FAR where there is no seed at all."""
    g = column_distance(seed)
    H, W = g.shape
    g2 = np.where(g >= NONE, NONE, g * g)
    x = np.arange(W, dtype=np.int64)
    dx2 = (x[:, None] - x[None, :]) ** 2                                               # [x][x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + g2[y][None, :]).min(axis=1)
    out = np.where(out >= NONE, FAR, out)
    if cap2 > 0:
        out = np.minimum(out, cap2)
    return out.astype(np.int32)


def brute_d2(seed):
    """The same by the definition alone: per pixel the minimum over all seeds (small rasters)."""
    s = np.asarray(seed) != 0
    H, W = s.shape
    ys, xs = np.nonzero(s)
    if ys.size == 0:
        return np.full((H, W), FAR, np.int32)
    y, x = np.mgrid[0:H, 0:W]
    d = (y[..., None] - ys) ** 2 + (x[..., None] - xs) ** 2
    return d.min(axis=-1).astype(np.int32)


def metres(d2, cellsize):
    """float32 [H][W]: one fp64 sqrt, one fp64 multiply, rounded to fp32 once; +inf at FAR."""
    d2 = np.asarray(d2)
    with np.errstate(over="ignore"):
        m = (np.float64(cellsize) * np.sqrt(d2.astype(np.float64))).astype(np.float32)
    return np.where(d2 == FAR, np.float32(np.inf), m)


def depth_px2(edges_m, cellsize):
    """Per edge the smallest integer t with sqrt(t) * cellsize >= edge in fp64, found by walking up from 0 in steps that
    cannot skip it (a bisection on the monotone predicate)."""
    out = []
    for e in edges_m:
        lo, hi = -1, 1                                  # predicate false at lo (or lo = -1), true at hi
        while math.sqrt(hi) * cellsize < e:
            lo, hi = hi, hi * 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if math.sqrt(mid) * cellsize >= e:
                hi = mid
            else:
                lo = mid
        out.append(0 if math.sqrt(0) * cellsize >= e else hi)
    return out


def depth_classes(sel_a, d2, class_d2, nclasses=8):
    """The raw numbers of tg_depth_errors from sel_a (|error| on the scored pixels, NaN elsewhere) and d2: per class the
    pixel count, fp64 sum a and sum a^2, and the bits of the largest a (0 for an empty class)."""
    a = np.asarray(sel_a, np.float32).ravel()
    d = np.asarray(d2).ravel().astype(np.int64)
    ok = ~np.isnan(a)
    cls = np.zeros(a.size, np.int64)
    for t in class_d2:
        cls += d >= int(t)
    counts, sum_a, sum_a2, max_bits = [], [], [], []
    for k in range(nclasses):
        v = a[ok & (cls == k)].astype(np.float64)
        counts.append(int(v.size))
        sum_a.append(float(np.sum(v)))
        sum_a2.append(float(np.sum(v * v)))
        max_bits.append(int(np.float32(v.max()).view(np.uint32)) if v.size else 0)
    return {"counts": counts, "sum_a": sum_a, "sum_a2": sum_a2, "max_bits": max_bits}


def hole_max_d2(labels, d2):
    """{label: the largest d2 over all pixels of the hole} for labels >= 0."""
    lab = np.asarray(labels).ravel()
    d = np.asarray(d2).ravel()
    out = {}
    for l in np.unique(lab[lab >= 0]):
        out[int(l)] = int(d[lab == l].max())
    return out
