"""fp64 numpy restatement of the raster resampling, independent of mvp_gan/src/resample.py.

The geometry of each axis is worked out in plain loops with fractions.Fraction, in source pixels (the product works in
integers of 1/q pixel); the two-dimensional sums run over numpy arrays, one step per tap of the footprint in row-major order,
because a 4x finer grid of even a small raster has a million pixels.

  scale(cellsize, target)                 the fraction p / q
  out_size(N, p, q)                       ceil(N q / p)
  area_axis / interp_axis                 per-axis taps and exact weights (Fractions)
  area(z, mask, nodata, p, q, cov, ...)   to a coarser grid
  interp(z, mask, nodata, p, q, ...)      to a finer grid
  back(work, z, mask, nodata, p, q)       the return trip with the known pixels passed through

area / interp return a dict: value float64 (NaN where unknown), known bool, n (taps of that pixel's formula), R (range of the
known taps it read), passed (bool, True where the keep raster's pixel was copied through)."""
from fractions import Fraction
from math import ceil, floor

import numpy as np


def known(z, mask=None, nodata=None):
    k = np.isfinite(z)
    if mask is not None:
        k &= np.asarray(mask) != 0
    if nodata is not None and not np.isnan(nodata):
        k &= z != np.float32(nodata)
    return k


def scale(cellsize, target):
    ratio = float(target) / float(cellsize)
    fr = Fraction(ratio).limit_denominator(64)
    if abs(float(fr) - ratio) > 1e-6 * ratio or not Fraction(1, 4) <= fr <= 16:
        raise ValueError((cellsize, target))
    return fr


def out_size(N, p, q):
    return ceil(Fraction(N * q, p))


def area_axis(N, p, q):
    """[(first source pixel, [overlap lengths in source pixels as Fractions])] per output pixel."""
    s = Fraction(p, q)
    out = []
    for I in range(out_size(N, p, q)):
        lo, hi = I * s, min((I + 1) * s, Fraction(N))
        i0, i1 = floor(lo), ceil(hi)
        out.append((i0, [min(Fraction(i + 1), hi) - max(Fraction(i), lo) for i in range(i0, i1)]))
    return out


def interp_axis(N, p, q):
    """[(4 clamped taps, 4 Catmull-Rom weights, 2 linear weights of taps[1:3], position 1 | 2 of the containing pixel)] per
    output pixel, weights as Fractions."""
    s = Fraction(p, q)
    out = []
    for I in range(out_size(N, p, q)):
        c = (I + Fraction(1, 2)) * s - Fraction(1, 2)              # centre in source pixel-centre coordinates
        f = floor(c)
        t = c - f
        cubic = [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2,
                 (t ** 3 - t ** 2) / 2]
        assert sum(cubic) == 1
        contain = floor((I + Fraction(1, 2)) * s)                  # the source pixel [i, i + 1) that holds the centre
        assert contain in (f, f + 1)
        out.append(([min(max(f - 1 + k, 0), N - 1) for k in range(4)], cubic, [1 - t, t], 1 + contain - f))
    return out


def _keep(keep, shape):
    if keep is None:
        return None, np.zeros(shape, bool)
    kz, km, knd = keep
    kz = np.asarray(kz, np.float32)[:shape[0], :shape[1]]
    km = None if km is None else np.asarray(km)[:shape[0], :shape[1]]
    return kz, known(kz, km, knd)


def area(z, mask=None, nodata=None, p=2, q=1, cov=Fraction(1, 2), keep=None, out_shape=None):
    """Area-weighted mean of the known taps; known iff the known share of the clipped footprint is positive and >= cov."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    k = known(z, mask, nodata)
    z64 = np.where(k, z, 0.0).astype(np.float64)
    rows, cols = area_axis(H, p, q), area_axis(W, p, q)
    if out_shape is not None:
        rows, cols = rows[:out_shape[0]], cols[:out_shape[1]]
    Ho, Wo = len(rows), len(cols)

    def pad(ax):
        T = max(len(w) for _, w in ax)
        idx = np.zeros((len(ax), T), np.int64)
        wgt = np.zeros((len(ax), T), np.int64)
        for I, (i0, w) in enumerate(ax):
            for t, wt in enumerate(w):
                idx[I, t] = i0 + t
                wi = wt * q
                assert wi.denominator == 1 and wi > 0
                wgt[I, t] = int(wi)
        return idx, wgt

    iy, wy = pad(rows)
    ix, wx = pad(cols)
    ct = np.zeros((Ho, Wo), np.int64)
    ck = np.zeros((Ho, Wo), np.int64)
    n = np.zeros((Ho, Wo), np.int64)
    have = np.zeros((Ho, Wo), bool)
    z0 = np.zeros((Ho, Wo))
    zmin, zmax = np.full((Ho, Wo), np.inf), np.full((Ho, Wo), -np.inf)
    taps = [(a, b) for a in range(iy.shape[1]) for b in range(ix.shape[1])]          # row-major
    for a, b in taps:
        w = wy[:, a, None] * wx[None, :, b]
        kk = k[np.ix_(iy[:, a], ix[:, b])] & (w > 0)
        zz = z64[np.ix_(iy[:, a], ix[:, b])]
        ct += w
        ck += np.where(kk, w, 0)
        n += w > 0
        first = kk & ~have
        z0 = np.where(first, zz, z0)
        have |= kk
        zmin = np.where(kk, np.minimum(zmin, zz), zmin)
        zmax = np.where(kk, np.maximum(zmax, zz), zmax)
    num = np.zeros((Ho, Wo))
    for a, b in taps:
        w = wy[:, a, None] * wx[None, :, b]
        kk = k[np.ix_(iy[:, a], ix[:, b])] & (w > 0)
        num += np.where(kk, w * (z64[np.ix_(iy[:, a], ix[:, b])] - z0), 0.0)
    cov = Fraction(cov)
    kn = (ck > 0) & (ck * cov.denominator >= cov.numerator * ct)
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where(kn, z0 + num / np.maximum(ck, 1), np.nan)
    kz, kk = _keep(keep, (Ho, Wo))
    if kz is not None:
        val = np.where(kk, kz.astype(np.float64), val)
        kn = kn | kk
    return {"value": val, "known": kn, "n": n, "R": np.where(have, zmax - zmin, 0.0), "passed": kk, "cov_known": ck,
            "cov_total": ct}


def interp(z, mask=None, nodata=None, p=1, q=2, keep=None, out_shape=None, rows=None, cols=None):
    """Bicubic where all 16 taps are known, else bilinear over the known ones of the 4 nearest; known iff the containing pixel
    is.  rows / cols: index arrays that restrict the output pixels computed (the result arrays then have their shape)."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    k = known(z, mask, nodata)
    z64 = np.where(k, z, 0.0).astype(np.float64)
    ay, ax = interp_axis(H, p, q), interp_axis(W, p, q)
    if out_shape is not None:
        ay, ax = ay[:out_shape[0]], ax[:out_shape[1]]
    full = (len(ay), len(ax))
    if rows is not None:
        ay = [ay[i] for i in rows]
    if cols is not None:
        ax = [ax[i] for i in cols]
    Ho, Wo = len(ay), len(ax)

    def arrays(ax_):
        return (np.array([t for t, _, _, _ in ax_], np.int64), np.array([[float(w) for w in c] for _, c, _, _ in ax_]),
                np.array([[float(w) for w in l] for _, _, l, _ in ax_]), np.array([c for _, _, _, c in ax_], np.int64))

    ty, cy, ly, py = arrays(ay)
    tx, cx, lx, px = arrays(ax)
    yc, xc = ty[np.arange(Ho), py], tx[np.arange(Wo), px]
    zc, kc = z64[np.ix_(yc, xc)], k[np.ix_(yc, xc)]
    all16 = np.ones((Ho, Wo), bool)
    for a in range(4):
        for b in range(4):
            all16 &= k[np.ix_(ty[:, a], tx[:, b])]
    bic, bil, S = np.zeros((Ho, Wo)), np.zeros((Ho, Wo)), np.zeros((Ho, Wo))
    mn16, mx16 = np.full((Ho, Wo), np.inf), np.full((Ho, Wo), -np.inf)
    mn4, mx4 = np.full((Ho, Wo), np.inf), np.full((Ho, Wo), -np.inf)
    for a in range(4):
        for b in range(4):
            zz, kk = z64[np.ix_(ty[:, a], tx[:, b])], k[np.ix_(ty[:, a], tx[:, b])]
            bic += cy[:, a, None] * cx[None, :, b] * (zz - zc)
            mn16, mx16 = np.where(kk, np.minimum(mn16, zz), mn16), np.where(kk, np.maximum(mx16, zz), mx16)
            if a in (1, 2) and b in (1, 2):
                w = ly[:, a - 1, None] * lx[None, :, b - 1]
                bil += np.where(kk, w * (zz - zc), 0.0)
                S += np.where(kk, w, 0.0)
                mn4, mx4 = np.where(kk, np.minimum(mn4, zz), mn4), np.where(kk, np.maximum(mx4, zz), mx4)
    assert (S[kc] > 0).all()
    with np.errstate(invalid="ignore", divide="ignore"):
        val = np.where(kc, np.where(all16, zc + bic, zc + bil / np.where(S > 0, S, 1.0)), np.nan)
    R = np.where(kc, np.where(all16, mx16 - mn16, mx4 - mn4), 0.0)
    kn = kc.copy()
    kz, kk = _keep(keep, full)
    if kz is not None:
        sel = np.ix_(np.arange(full[0]) if rows is None else np.asarray(rows), np.arange(full[1]) if cols is None else np.asarray(cols))
        kz, kk = kz[sel], kk[sel]
        val = np.where(kk, kz.astype(np.float64), val)
        kn = kn | kk
    else:
        kk = np.zeros((Ho, Wo), bool)
    return {"value": val, "known": kn, "n": np.where(all16, 16, 4), "R": R, "passed": kk, "bicubic": all16 & kc}


def back(work, z, mask=None, nodata=None, p=2, q=1):
    """The return trip from the working grid of scale p / q to z's grid: the other operator at q / p, cropped to z's shape, any
    finite working pixel making an area mean, z's known pixels passed through."""
    z = np.asarray(z, np.float32)
    assert tuple(np.shape(work)) == (out_size(z.shape[0], p, q), out_size(z.shape[1], p, q))
    if p >= q:
        return interp(work, None, None, q, p, keep=(z, mask, nodata), out_shape=z.shape)
    return area(work, None, None, q, p, cov=0, keep=(z, mask, nodata), out_shape=z.shape)
