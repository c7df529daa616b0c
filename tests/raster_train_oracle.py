"""numpy oracle of the training-window kernels (csrc/raster_train.hip): hole masks from integer primitives in int64, and
windows cut under a dihedral transform and min-max normalised in float32.  The kernels must match both bit for bit.
Independent of mvp_gan/src/utils/raster_dataset.py."""
import numpy as np

RECT, ELLIPSE, STROKE = 0, 1, 2


def cover(prim, side):
    """bool [side][side]: the pixels one primitive (8 ints, terragan_hip.h) makes a hole."""
    k = int(prim[0])
    i, j = np.meshgrid(np.arange(side, dtype=np.int64), np.arange(side, dtype=np.int64), indexing="ij")
    p = [int(v) for v in prim]
    if k == STROKE:
        y0, x0, y1, x1, r = p[1:6]
        wy, wx, dy, dx = i - y0, j - x0, y1 - y0, x1 - x0
        wd, dd, r2 = wy * dy + wx * dx, dy * dy + dx * dx, r * r
        near = wy * wy + wx * wx <= r2
        far = (i - y1) ** 2 + (j - x1) ** 2 <= r2
        mid = (wy * dx - wx * dy) ** 2 <= r2 * dd
        return np.where(wd <= 0, near, np.where(wd >= dd, far, mid))
    if k not in (RECT, ELLIPSE):
        return np.zeros((side, side), bool)
    cy, cx, a, b, u, v = p[1:7]
    l2 = u * u + v * v
    if l2 == 0 or (k == ELLIPSE and (a == 0 or b == 0)):
        return np.zeros((side, side), bool)
    dy, dx = i - cy, j - cx
    pp, qq = dx * u + dy * v, dy * u - dx * v
    if k == RECT:
        return (pp * pp <= a * a * l2) & (qq * qq <= b * b * l2)
    return pp * pp * (b * b) + qq * qq * (a * a) <= a * a * b * b * l2


def hole_masks(prims, offsets, side):
    """float32 [n][side][side], 1 = keep, 0 = hole (at most 32 primitives of a window are used, as in the kernel)."""
    prims, offsets = np.asarray(prims).reshape(-1, 8), np.asarray(offsets)
    n = len(offsets) - 1
    out = np.ones((n, side, side), np.float32)
    for w in range(n):
        a, b = int(offsets[w]), int(offsets[w + 1])
        for q in range(a, min(b, a + 32)):
            out[w][cover(prims[q], side)] = 0
    return out


def transform(win, op):
    """Output of a source window [side][side] under dihedral op: out[i][j] = win[a][b] (terragan_hip.h)."""
    t = win.T if op & 4 else win
    if op & 2:
        t = t[::-1, :] if not op & 4 else t[:, ::-1]
    if op & 1:
        t = t[:, ::-1] if not op & 4 else t[::-1, :]
    return np.ascontiguousarray(t)


def transform_ref(win, op):
    """transform() spelled out pixel by pixel (the definition the fast form above is checked against)."""
    side = win.shape[0]
    out = np.empty_like(win)
    for i in range(side):
        for j in range(side):
            a, b = (j, i) if op & 4 else (i, j)
            a = side - 1 - a if op & 2 else a
            b = side - 1 - b if op & 1 else b
            out[i, j] = win[a, b]
    return out


def sample(dem, draws, mask, norm_known=True):
    """-> x float32 [n][side][side], lo, hi float32 [n] (tg_raster_sample)."""
    draws, mask = np.asarray(draws).reshape(-1, 3), np.asarray(mask, np.float32)
    n, side = mask.shape[0], mask.shape[1]
    H, W = dem.shape
    x = np.empty((n, side, side), np.float32)
    lo, hi = np.empty(n, np.float32), np.empty(n, np.float32)
    for w, (y0, x0, op) in enumerate(draws.tolist()):
        if y0 < 0 or x0 < 0 or y0 + side > H or x0 + side > W or not 0 <= op <= 7:
            x[w], lo[w], hi[w] = np.nan, np.nan, np.nan
            continue
        z = transform(dem[y0:y0 + side, x0:x0 + side], op)
        sel = z[mask[w] != 0] if norm_known else z.ravel()
        if sel.size == 0:
            lo[w], hi[w], x[w] = np.inf, -np.inf, 0
            continue
        lo[w], hi[w] = sel.min() + np.float32(0), sel.max() + np.float32(0)      # + 0: a -0 extreme becomes +0
        if lo[w] < hi[w]:
            with np.errstate(over="ignore"):
                x[w] = (z - lo[w]) / (hi[w] - lo[w])
        else:
            x[w] = 0
    return x, lo, hi
