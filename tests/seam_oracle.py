"""numpy fp64 oracle of the seam correction (mvp_gan/src/seam_correct.py, csrc/seam.hip): ring, ring targets, the delta raster,
its harmonic completion through tests/vfill_oracle.py, and the corrected raster.  Independent of the package."""
import numpy as np

from tests import vfill_oracle as VO

DIRS = ((-1, 0), (0, -1), (0, 1), (1, 0))          # up, left, right, down


def classify(z, filled, mask=None, nodata=None):
    """-> known, ring, interior, unfilled (bool [H][W])."""
    z = np.asarray(z)
    H, W = z.shape
    k = VO.known_mask(z, mask, nodata)
    fin = np.isfinite(np.asarray(filled)) & ~k
    near = np.zeros((H, W), bool)
    near[1:, :] |= k[:-1, :]
    near[:-1, :] |= k[1:, :]
    near[:, 1:] |= k[:, :-1]
    near[:, :-1] |= k[:, 1:]
    return k, fin & near, fin & ~near, ~k & ~fin


def delta(z, filled, mask=None, nodata=None, order=1):
    """-> (D float64 [H][W]: the ring target minus the fill on the ring, 0 on the known pixels and the unfilled holes, NaN on the
    interior; known, ring, interior, unfilled)."""
    z64 = np.asarray(z).astype(np.float64)
    g64 = np.asarray(filled).astype(np.float64)
    H, W = z64.shape
    k, ring, interior, unfilled = classify(z, filled, mask, nodata)
    D = np.zeros((H, W))
    D[interior] = np.nan
    for y, x in np.argwhere(ring):
        acc, n = 0.0, 0
        for dy, dx in DIRS:
            qy, qx = y + dy, x + dx
            if not (0 <= qy < H and 0 <= qx < W and k[qy, qx]):
                continue
            e = z64[qy, qx]
            ry, rx = qy + dy, qx + dx
            if order == 1 and 0 <= ry < H and 0 <= rx < W and k[ry, rx]:
                e = 2.0 * z64[qy, qx] - z64[ry, rx]
            acc += e - g64[y, x]
            n += 1
        D[y, x] = acc / n
    return D, k, ring, interior, unfilled


def correct(z, filled, mask=None, nodata=None, order=1):
    """-> (raster float64 [H][W], info: ring, interior, unfilled, max_delta, D (before the solve), known)."""
    D, k, ring, interior, unfilled = delta(z, filled, mask, nodata, order)
    g64 = np.asarray(filled).astype(np.float64)
    if ring.any():
        Ds = VO.solve(D, ~interior)
    else:
        Ds = np.zeros_like(D)                       # no rim: the fill is returned as it is
    out = np.full(D.shape, np.nan)
    out[k] = np.asarray(z).astype(np.float64)[k]
    f = ring | interior
    out[f] = g64[f] + Ds[f]
    info = {"ring": int(ring.sum()), "interior": int(interior.sum()), "unfilled": int(unfilled.sum()),
            "max_delta": float(np.abs(D[ring]).max()) if ring.any() else 0.0, "D": D, "known": k}
    return out, info


def ring8(known, scored):
    """`scored` pixels with an 8-neighbour in `known` (the ring of evaluate_raster)."""
    H, W = known.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = known
    near = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                near |= p[dy:dy + H, dx:dx + W]
    return scored & near
