"""numpy oracle of whole-raster inpainting (csrc/raster.hip): window stats and gather in float32 (the kernels must match
them bit for bit), blend in float64.  Independent of mvp_gan/src/inpaint_raster.py except for the window plan."""
import numpy as np


def known(z, mask=None, nodata=None):
    k = np.isfinite(z)
    if mask is not None:
        k &= mask != 0
    if nodata is not None:
        k &= z != np.float32(nodata)
    return k


def windows(plan):
    """[(row0, col0)] in window-index order (row-major over the window grid)."""
    return [(y0, x0) for y0 in plan.ys for x0 in plan.xs]


def stats(z, plan, mask=None, nodata=None):
    """-> lo, hi (float32 [nwin]), counts int32 [nwin][2] (known, holes)."""
    k = known(z, mask, nodata)
    lo, hi, cnt = [], [], []
    for y0, x0 in windows(plan):
        zw, kw = z[y0:y0 + plan.wh, x0:x0 + plan.ww], k[y0:y0 + plan.wh, x0:x0 + plan.ww]
        n = int(kw.sum())
        cnt.append((n, kw.size - n))
        lo.append(zw[kw].min() + np.float32(0) if n else np.float32(0))      # + 0: -0 extremes become +0
        hi.append(zw[kw].max() + np.float32(0) if n else np.float32(0))
    return np.array(lo, np.float32), np.array(hi, np.float32), np.array(cnt, np.int32)


def gather(z, plan, lo, hi, win_idx, mask=None, nodata=None):
    """-> x, m float32 [n][wh][ww]: x = (z - lo) / (hi - lo) at known pixels (IEEE fp32), else 0; 0 when hi == lo."""
    k = known(z, mask, nodata)
    wins = windows(plan)
    xs, ms = [], []
    for j in win_idx:
        y0, x0 = wins[j]
        zw, kw = z[y0:y0 + plan.wh, x0:x0 + plan.ww], k[y0:y0 + plan.wh, x0:x0 + plan.ww]
        l, h = np.float32(lo[j]), np.float32(hi[j])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            x = (zw - l) / (h - l) if h != l else np.zeros_like(zw)
        xs.append(np.where(kw, x, np.float32(0)).astype(np.float32))
        ms.append(kw.astype(np.float32))
    return np.stack(xs), np.stack(ms)


def ramp(w, overlap, first, last):
    t = np.arange(w, dtype=np.float64)
    r = np.ones(w)
    if overlap:
        if not first:
            r = np.minimum(r, (t + 0.5) / overlap)
        if not last:
            r = np.minimum(r, (w - t - 0.5) / overlap)
    return r


def blend(z, plan, lo, hi, run_of_window, wout, mask=None, nodata=None):
    """float64 composite: known pixels = z, holes = weighted mean of lo + out * (hi - lo) over the running covering
    windows, NaN where none covers.  -> (raster float64 [H][W], unfilled count)."""
    k = known(z, mask, nodata)
    num = np.zeros(z.shape)
    den = np.zeros(z.shape)
    for j, (y0, x0) in enumerate(windows(plan)):
        r = run_of_window[j]
        if r < 0:
            continue
        wy = ramp(plan.wh, plan.overlap, y0 == 0, y0 + plan.wh == plan.H)
        wx = ramp(plan.ww, plan.overlap, x0 == 0, x0 + plan.ww == plan.W)
        w = wy[:, None] * wx[None, :]
        l, h = float(lo[j]), float(hi[j])
        num[y0:y0 + plan.wh, x0:x0 + plan.ww] += w * (l + wout[r].astype(np.float64) * (h - l))
        den[y0:y0 + plan.wh, x0:x0 + plan.ww] += w
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(den > 0, num / den, np.nan)
    out = np.where(k, z.astype(np.float64), out)
    return out, int((~k & (den == 0)).sum())


def disc_holes(H, W, frac, seed, rmin=8, rmax=40):
    """bool [H][W], True = hole: random discs until about `frac` of the pixels are holes."""
    rng = np.random.default_rng(seed)
    hole = np.zeros((H, W), bool)
    while hole.mean() < frac:
        for _ in range(16):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(rmin, rmax + 1)
            y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
            yy, xx = np.ogrid[y0:y1, x0:x1]
            hole[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return hole


def terrain(H, W, seed, base=850.0, relief=120.0):
    """Smooth synthetic DSM in metres, float32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    z = np.zeros((H, W))
    for _ in range(6):
        fy, fx, ph = rng.uniform(0.002, 0.03), rng.uniform(0.002, 0.03), rng.uniform(0, 6.3)
        z += rng.uniform(0.3, 1.0) * np.sin(fy * yy + ph) * np.cos(fx * xx - ph)
    z = (z - z.min()) / (z.max() - z.min())
    return (base + relief * z + rng.normal(0, 0.3, (H, W))).astype(np.float32)
