"""numpy oracle of the object detector (csrc/objmask.hip, mvp_gan/src/object_mask.py), and the seeded synthetic scene that
tests/test_hip_object_mask.py and tools/object_mask_bench.py share.  numpy only: the GPU machine may not have scipy."""
import numpy as np


def morph1d(a, r, axis, op):
    """op (np.minimum / np.maximum) over the clipped window [i - r, i + r] along `axis`, by shifted op with doubling spans."""
    ident = np.inf if op is np.minimum else -np.inf
    a = np.moveaxis(np.asarray(a, np.float32), axis, 0)
    N = a.shape[0]
    r = min(int(r), N - 1)
    k = 2 * r + 1
    pad = np.full((N + 2 * r,) + a.shape[1:], ident, np.float32)
    pad[r:r + N] = a
    span, A = 1, pad                       # A[i] = op over pad[i : i + span]
    while 2 * span <= k:
        A = op(A[:-span], A[span:])
        span *= 2
    out = op(A[:N], A[k - span:k - span + N])
    return np.moveaxis(out, 0, axis)


def morph(z, known, r, op):
    """op over the known pixels of the clipped (2r+1)^2 window; +inf (min) / -inf (max) where there is none."""
    ident = np.inf if op is np.minimum else -np.inf
    x = np.where(known, np.asarray(z, np.float32), np.float32(ident)).astype(np.float32)
    return morph1d(morph1d(x, r, 1, op), r, 0, op)


def morph_brute(z, known, r, op):
    H, W = z.shape
    ident = np.inf if op is np.minimum else -np.inf
    out = np.empty((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, H), max(x - r, 0), min(x + r + 1, W)
            v = z[y0:y1, x0:x1][known[y0:y1, x0:x1]]
            out[y, x] = op.reduce(v) if v.size else ident
    return out


def known_map(z, mask=None, nodata=None):
    k = np.isfinite(z)
    if mask is not None:
        k &= np.asarray(mask) != 0
    if nodata is not None and not np.isnan(nodata):
        k &= z != np.float32(nodata)
    return k


def pmf(z, known, radii, thresholds):
    """-> (flags bool [H][W], final surface float32): s_{k+1} = dilate(erode(s_k)) over the known pixels."""
    s = np.asarray(z, np.float32)
    flags = np.zeros(s.shape, bool)
    for r, dh in zip(radii, thresholds):
        e = morph(s, known, r, np.minimum)
        d = morph(e, known, r, np.maximum)
        with np.errstate(invalid="ignore"):
            flags |= known & ((s - d).astype(np.float32) > np.float32(dh))
        s = d
    return flags, s


def components(flags):
    """8-connected labels: the smallest linear index of each component, -1 off the flags (min hooking + pointer jumping)."""
    H, W = flags.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    par = np.where(flags, idx, -1).ravel()
    edges = []
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        ys, ye = 0, H - dy
        xs, xe = max(0, -dx), W - max(0, dx)
        a = flags[ys:ye, xs:xe] & flags[ys + dy:ye + dy, xs + dx:xe + dx]
        p, q = idx[ys:ye, xs:xe][a], idx[ys + dy:ye + dy, xs + dx:xe + dx][a]
        edges.append((p, q))
    p = np.concatenate([e[0] for e in edges]) if edges else np.zeros(0, np.int64)
    q = np.concatenate([e[1] for e in edges]) if edges else np.zeros(0, np.int64)
    while True:
        rp, rq = par[p], par[q]
        diff = rp != rq
        if not diff.any():
            break
        lo, hi = np.minimum(rp[diff], rq[diff]), np.maximum(rp[diff], rq[diff])
        np.minimum.at(par, hi, lo)                 # hook the larger root under the smaller
        while True:                                 # pointer jumping to the roots
            nxt = np.where(par >= 0, par[np.maximum(par, 0)], -1)
            if (nxt == par).all():
                break
            par = nxt
    return par.reshape(H, W)


def areas(labels):
    a = np.zeros(labels.size, np.int64)
    lab = labels.ravel()
    np.add.at(a, lab[lab >= 0], 1)
    return a


def filter_buffer(known, labels, min_area, buffer_px):
    """-> (objects uint8, keep float32, counts [flagged, kept, removed, object pixels])."""
    a = areas(labels)
    lab = labels
    obj = (lab >= 0) & (a[np.maximum(lab, 0)] >= min_area)
    o = morph1d(morph1d(obj.astype(np.float32), buffer_px, 1, np.maximum), buffer_px, 0, np.maximum) > 0
    keep = (known & ~o).astype(np.float32)
    roots = lab.ravel() == np.arange(lab.size)
    counts = [int((lab >= 0).sum()), int((roots & (a >= min_area)).sum()), int((roots & (a < min_area)).sum()), int(o.sum())]
    return o.astype(np.uint8), keep, counts


def object_mask(z, known, radii, thresholds, min_area, buffer_px):
    flags, s = pmf(z, known, radii, thresholds)
    labels = components(flags)
    o, keep, counts = filter_buffer(known, labels, min_area, buffer_px)
    return o, keep, counts, flags, s, labels


# ---- seeded synthetic scene -------------------------------------------------------------------------------------------
def scene(H=2048, W=2048, seed=0, buildings=None, trees=None):
    """-> (dsm float32 [H][W] in metres at 1 m cells, truth bool [H][W] = building or tree footprint).
    Ground: a plane of slope <= 0.1 m/m, hills of <= 10 m amplitude at >= 500 m wavelength, 5 cm noise.  On it, axis-aligned
    flat-roofed buildings of 8-40 m sides and 4-15 m height, and dome trees of 2-6 m radius and 4-12 m height."""
    rng = np.random.default_rng(seed)
    nb = buildings if buildings is not None else max(100, H * W // 30000)
    nt = trees if trees is not None else max(200, H * W // 15000)
    y, x = np.arange(H, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    gy, gx = rng.uniform(-0.07, 0.07, 2)
    ground = 100.0 + gy * y + gx * x
    for _ in range(3):
        amp, lam = rng.uniform(2.0, 10.0 / 3), rng.uniform(500.0, 1500.0)
        th, ph = rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
        ground = ground + amp * np.sin(2 * np.pi * (np.cos(th) * x + np.sin(th) * y) / lam + ph)
    ground = ground + rng.normal(0.0, 0.05, (H, W))
    add = np.zeros((H, W), np.float64)
    for _ in range(nb):
        h, w = rng.integers(8, 41, 2)
        y0, x0 = rng.integers(0, H - h + 1), rng.integers(0, W - w + 1)
        base = ground[y0:y0 + h, x0:x0 + w].max()
        roof = base + rng.uniform(4.0, 15.0) - ground[y0:y0 + h, x0:x0 + w]
        add[y0:y0 + h, x0:x0 + w] = np.maximum(add[y0:y0 + h, x0:x0 + w], roof)
    for _ in range(nt):
        R, ht = rng.uniform(2.0, 6.0), rng.uniform(4.0, 12.0)
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        y0, y1 = max(int(cy - R), 0), min(int(cy + R) + 2, H)
        x0, x1 = max(int(cx - R), 0), min(int(cx + R) + 2, W)
        d2 = ((np.arange(y0, y1)[:, None] + 0.5 - cy) ** 2 + (np.arange(x0, x1)[None, :] + 0.5 - cx) ** 2) / (R * R)
        dome = np.where(d2 < 1, ht * np.sqrt(np.maximum(1 - d2, 0)), 0.0)
        add[y0:y1, x0:x1] = np.maximum(add[y0:y1, x0:x1], dome)
    return (ground + add).astype(np.float32), add > 0
