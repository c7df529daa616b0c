"""numpy oracle of the held-out terrain errors (csrc/terrain_eval.hip, mvp_gan/src/evaluate_raster.py): evaluation holes,
Horn gradients and Laplacians, the raw counts, sums, per-hole table and quantiles, and the report built from them."""
import math

import numpy as np

from tests import objmask_oracle as OM
from tests import raster_train_oracle as RT

FIX, CLAMP = 2.0 ** 16, 2.0 ** 15


def valid_map(z, mask=None, nodata=None):
    return OM.known_map(z, mask, nodata)


def cell_hole_map(H, W, split, block, tile, holes, seed):
    """bool [H][W]: the hole pixels of the eligible cells (primitives by evaluate_raster's cell plan, rasterised by the numpy
    tg_hole_masks oracle), clipped to the raster."""
    from mvp_gan.src.evaluate_raster import cell_primitives, eligible_cells
    el = eligible_cells(H, W, split, block, tile)
    out = np.zeros((H, W), bool)
    cells = np.argwhere(el).tolist()
    if not cells:
        return out
    prims, offsets = cell_primitives(seed, split, cells, tile, holes)
    masks = RT.hole_masks(prims, offsets, tile)
    for k, (cy, cx) in enumerate(cells):
        y0, x0 = cy * tile, cx * tile
        h, w = min(tile, H - y0), min(tile, W - x0)
        out[y0:y0 + h, x0:x0 + w] = masks[k, :h, :w] == 0
    return out


def eval_holes(z, mask, nodata, objects, hole):
    """-> (holes uint8, keep float32, [valid, holes, valid object pixels])."""
    v = valid_map(z, mask, nodata)
    o = np.zeros(z.shape, bool) if objects is None else np.asarray(objects) != 0
    hol = v & hole & ~o
    keep = v & ~hole & ~o
    return hol.astype(np.uint8), keep.astype(np.float32), [int(v.sum()), int(hol.sum()), int((v & o).sum())]


def horn(z, c):
    """-> (gx, gy, lap) float64 [H-2][W-2] at the interior pixels."""
    z = np.asarray(z, np.float64)
    a, b, cc = z[:-2, :-2], z[:-2, 1:-1], z[:-2, 2:]
    d, e, f = z[1:-1, :-2], z[1:-1, 1:-1], z[1:-1, 2:]
    g, h, k = z[2:, :-2], z[2:, 1:-1], z[2:, 2:]
    gx = ((cc + 2.0 * f + k) - (a + 2.0 * d + g)) / (8.0 * c)
    gy = ((g + 2.0 * h + k) - (a + 2.0 * b + cc)) / (8.0 * c)
    lap = (b + h + d + f - 4.0 * e) / (c * c)
    return gx, gy, lap


def slope_deg(gx, gy):
    return np.degrees(np.arctan(np.hypot(gx, gy)))


def _shift_any(m):
    """bool: any 8-neighbour (inside the raster) of each pixel is set in m."""
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                out |= p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return out


def _shift_all(m):
    """bool: the whole 3x3 neighbourhood lies inside the raster and is set in m."""
    H, W = m.shape
    out = np.zeros((H, W), bool)
    if H < 3 or W < 3:
        return out
    a = np.ones((H - 2, W - 2), bool)
    for dy in range(3):
        for dx in range(3):
            a &= m[dy:dy + H - 2, dx:dx + W - 2]
    out[1:-1, 1:-1] = a
    return out


def raw(z, p, holes, keep, c, mask=None, nodata=None, edges_m2=(100.0, 1000.0, 10000.0)):
    """-> dict: counts (evaluate_raster.COUNTS), sums (SUMS + class_a / class_a2), table int64 [n][9] sorted by label,
    sel_a (a over S), sel_s (float32 |slope error| over T), and the pixel sets."""
    from mvp_gan.src.evaluate_raster import class_px
    z, p = np.asarray(z, np.float32), np.asarray(p, np.float32)
    H, W = z.shape
    v = valid_map(z, mask, nodata)
    hol = np.asarray(holes) != 0
    K = np.asarray(keep) != 0
    pf = np.isfinite(p)
    S = hol & pf
    with np.errstate(invalid="ignore", over="ignore"):
        e = (p - z).astype(np.float32)
    a = np.abs(e)
    T = S & _shift_all(v & pf)
    R = S & _shift_any(K)
    ds = np.zeros((H, W)); dg2 = np.zeros((H, W)); dl = np.zeros((H, W))
    if H >= 3 and W >= 3:
        with np.errstate(invalid="ignore", over="ignore"):
            gz, gp = horn(np.where(v, z, 0), c), horn(np.where(pf, p, 0), c)
            ds[1:-1, 1:-1] = slope_deg(gp[0], gp[1]) - slope_deg(gz[0], gz[1])
            dg2[1:-1, 1:-1] = (gp[0] - gz[0]) ** 2 + (gp[1] - gz[1]) ** 2
            dl[1:-1, 1:-1] = gp[2] - gz[2]
    ad = a.astype(np.float64)
    labels = OM.components(hol)
    areas = OM.areas(labels)
    roots = np.flatnonzero(labels.ravel() == np.arange(H * W))
    px = class_px(edges_m2, c)
    cls_of_root = np.zeros(roots.size, np.int64)
    for t in px:
        cls_of_root += areas[roots] >= t
    idx = np.searchsorted(roots, np.maximum(labels.ravel(), 0)).reshape(H, W)
    pix_cls = np.where(hol, cls_of_root[np.minimum(idx, max(roots.size - 1, 0))] if roots.size else 0, -1)
    counts = {"valid": int(v.sum()), "holes": int(hol.sum()), "objects": int((v & ~hol & ~K).sum()), "scored": int(S.sum()),
              "unfilled": int((hol & ~pf).sum()), "ring": int(R.sum()), "slope_scored": int(T.sum()),
              "ring_slope": int((R & T).sum()), "clamped": int((S & (a > CLAMP)).sum()),
              "max_bits": int(a[S].max().view(np.uint32)) if S.any() else 0}
    sums = {"s_e": e[S].astype(np.float64).sum(), "s_a": ad[S].sum(), "s_a2": (ad[S] ** 2).sum(),
            "t_ds": np.abs(ds[T]).sum(), "t_ds2": (ds[T] ** 2).sum(), "t_dg2": dg2[T].sum(), "t_dl2": (dl[T] ** 2).sum(),
            "r_a": ad[R].sum(), "r_a2": (ad[R] ** 2).sum(), "rt_dg2": dg2[R & T].sum(),
            "class_a": [ad[S & (pix_cls == k)].sum() for k in range(len(edges_m2) + 1)],
            "class_a2": [(ad[S & (pix_cls == k)] ** 2).sum() for k in range(len(edges_m2) + 1)]}
    fixed = np.rint(np.minimum(np.where(S, ad, 0.0), CLAMP) * FIX).astype(np.int64)
    table = np.zeros((roots.size, 9), np.int64)
    ys, xs = np.divmod(np.arange(H * W).reshape(H, W), W)
    for j, r in enumerate(roots):
        m = labels == r
        sm = m & S
        table[j] = [r, areas[r], sm.sum(), fixed[sm].sum(), a[sm].max().view(np.uint32) if sm.any() else 0,
                    ys[m].min(), xs[m].min(), ys[m].max(), xs[m].max()]
    sel_a = np.where(S, a, np.float32(np.nan)).astype(np.float32)
    sel_s = np.where(T, np.abs(ds).astype(np.float32), np.float32(np.nan)).astype(np.float32)
    return {"counts": counts, "sums": sums, "table": table, "sel_a": sel_a, "sel_s": sel_s, "S": S, "T": T, "R": R,
            "labels": labels}


def nearest_rank(vals, qs):
    from mvp_gan.src.evaluate_raster import rank
    v = np.sort(vals[~np.isnan(vals)])
    return [float(v[rank(q, v.size)]) if v.size else math.nan for q in qs]


def report(z, p, holes, keep, c, mask=None, nodata=None, edges_m2=(100.0, 1000.0, 10000.0), quantiles=(0.5, 0.9, 0.95, 0.99),
           top=10):
    from mvp_gan.src.evaluate_raster import assemble_report
    r = raw(z, p, holes, keep, c, mask, nodata, edges_m2)
    qa = nearest_rank(r["sel_a"], quantiles)
    qs = nearest_rank(r["sel_s"], (0.9,))[0]
    return assemble_report(r["counts"], r["sums"], r["table"], qa, qs, cellsize=c, edges_m2=list(edges_m2),
                           quantiles=list(quantiles), top=top), r
