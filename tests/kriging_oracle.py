"""numpy fp64 oracle of the empirical semivariogram and of ordinary kriging over the eight ray hits (csrc/kriging.hip,
mvp_gan/src/kriging.py).  Written from the definitions: the variogram by slicing, the kriging weights from
the bordered (n + 1) x (n + 1) system by np.linalg.solve, with the weights, the multiplier and the system's 2-norm condition number
for the bounds of tests/test_hip_kriging.py.  reduced() is the algebra the kernel uses (elimination against the nearest sample,
Cholesky), kept apart so that the two can be checked against each other without a GPU.  The ray hits are tests/idw_oracle.py's."""
import math

import numpy as np

from tests.idw_oracle import DIRS, SCALE, nearest, ray_hits  # noqa: F401  (re-exported for the tests)

OCTAVES = 6
EPS = 2.0 ** -52


# ---- the empirical variogram ------------------------------------------------------------------------------------------------
def variogram(z, known, octaves=OCTAVES):
    """-> (pairs int64 [2 * octaves], sums float64 [2 * octaves]: math.fsum of d * d, d = float64(z_a) - float64(z_b)), scale
    2 j + cls: cls 0 the steps (0, L) and (L, 0), cls 1 (L, L) and (L, -L), L = 2^j; both pixels known."""
    z = np.asarray(z, np.float32).astype(np.float64)
    kn = np.asarray(known) != 0
    H, W = kn.shape
    pairs, sums = np.zeros(2 * octaves, np.int64), np.zeros(2 * octaves, np.float64)
    for j in range(octaves):
        L = 1 << j
        a = lambda ys, xs: (z[ys, xs], kn[ys, xs])
        lo_y, hi_y = slice(0, max(H - L, 0)), slice(min(L, H), H)
        lo_x, hi_x = slice(0, max(W - L, 0)), slice(min(L, W), W)
        full = slice(None)
        steps = {0: [((full, lo_x), (full, hi_x)), ((lo_y, full), (hi_y, full))],
                 1: [((lo_y, lo_x), (hi_y, hi_x)), ((lo_y, hi_x), (hi_y, lo_x))]}
        for cls, lst in steps.items():
            terms = []
            for pa, pb in lst:
                (za, ka), (zb, kb) = a(*pa), a(*pb)
                both = ka & kb
                d = za[both] - zb[both]
                terms.append(d * d)
                pairs[2 * j + cls] += int(both.sum())
            sums[2 * j + cls] = math.fsum(np.concatenate(terms).tolist())
    return pairs, sums


def pair_counts_full(H, W, octaves=OCTAVES):
    """The closed form for a fully known raster."""
    out = []
    for j in range(octaves):
        L = 1 << j
        out += [H * max(W - L, 0) + max(H - L, 0) * W, 2 * max(H - L, 0) * max(W - L, 0)]
    return np.array(out, np.int64)


# ---- one kriging system -----------------------------------------------------------------------------------------------------
def _gammas(off, vg, cellsize):
    """off int64 [P][n][2] -> (Gamma [P][n][n], gamma0 [P][n]) from the exact squared pixel distances."""
    off = np.asarray(off, np.int64)
    d = off[:, :, None, :] - off[:, None, :, :]
    n2 = (d * d).sum(-1)
    n0 = (off * off).sum(-1)
    c = np.float64(cellsize)
    return vg.gamma(c * np.sqrt(n2.astype(np.float64))), vg.gamma(c * np.sqrt(n0.astype(np.float64)))


def bordered(off, zs, vg, cellsize):
    """P configurations of n >= 1 samples at the pixel offsets off [P][n][2] with the heights zs [P][n] -> dict of float64 arrays:
    est = sum w z, var = sum w gamma_0 + mu, w [P][n], mu, cond (2-norm, of the bordered matrix), absw_z = sum |w z|,
    absw_g = sum |w| gamma_0 + |mu|."""
    off = np.asarray(off, np.int64)
    zs = np.asarray(zs, np.float64)
    P, n = zs.shape
    G, g0 = _gammas(off, vg, cellsize)
    A = np.zeros((P, n + 1, n + 1), np.float64)
    A[:, :n, :n] = G
    A[:, :n, n] = 1.0
    A[:, n, :n] = 1.0
    rhs = np.concatenate([g0, np.ones((P, 1))], axis=1)
    sol = np.linalg.solve(A, rhs[:, :, None])[:, :, 0]
    w, mu = sol[:, :n], sol[:, n]
    return {"est": (w * zs).sum(1), "var": (w * g0).sum(1) + mu, "w": w, "mu": mu, "cond": np.linalg.cond(A),
            "absw_z": np.abs(w * zs).sum(1), "absw_g": (np.abs(w) * g0).sum(1) + np.abs(mu)}


def reduced(off, zs, vg, cellsize):
    """The same estimates by the kernel's algebra, one configuration: r = the nearest sample (the first among equals),
    M_ij = gamma_ir + gamma_jr - gamma_ij, b_i = gamma_ir + gamma_r0 - gamma_i0 over the other samples, Cholesky, est = z_r +
    sum w_i (z_i - z_r), var = max(0, 2 gamma_r0 - b^T M^-1 b).  -> (est, var, w [n] in the order of off)."""
    off = np.asarray(off, np.int64)
    zs = np.asarray(zs, np.float64)
    n = len(zs)
    G, g0 = _gammas(off[None], vg, cellsize)
    G, g0 = G[0], g0[0]
    r = int(np.argmin((off * off).sum(-1)))                  # argmin returns the first minimum
    rest = [i for i in range(n) if i != r]
    if not rest:
        return float(zs[r]), float(2.0 * g0[r]), np.ones(1)
    M = G[rest, r][:, None] + G[rest, r][None, :] - G[np.ix_(rest, rest)]
    b = G[rest, r] + g0[r] - g0[rest]
    Lc = np.linalg.cholesky(M)
    c = np.linalg.solve(Lc, b)
    y = np.linalg.solve(Lc.T, c)
    w = np.zeros(n)
    w[rest] = y
    w[r] = 1.0 - y.sum()
    return float(zs[r] + (y * (zs[rest] - zs[r])).sum()), max(0.0, float(2.0 * g0[r] - (c * c).sum())), w


# ---- a raster ---------------------------------------------------------------------------------------------------------------
def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def krige(z, known, hits, vg, cellsize, d2=None, idx=None):
    """-> dict: out, var float64 [H][W] (known: z and 0; NaN where nothing serves), est_bound, var_bound float64 [H][W]: the
    bounds of the issue per void pixel, 0.5 ulp32(oracle) + 64 * 2^-52 * cond * (sum |w z|, or sum |w| gamma_0 + |mu|), 0 on known
    pixels; counts [by rays, by nearest, left NaN]; nhits int [H][W].  The pixels are solved in batches that share a hit
    pattern."""
    z = np.asarray(z, np.float32)
    kn = np.asarray(known) != 0
    H, W = kn.shape
    hits = np.asarray(hits).astype(np.int64)
    out = np.where(kn, z.astype(np.float64), np.nan)
    var = np.where(kn, 0.0, np.nan)
    eb, vb = np.zeros((H, W)), np.zeros((H, W))
    have = (hits > 0) & ~kn[None]
    pattern = (have * (1 << np.arange(8))[:, None, None]).sum(0)
    dirs = np.array(DIRS, np.int64)
    for pat in np.unique(pattern[~kn]):
        if pat == 0:
            continue
        ys, xs = np.nonzero((pattern == pat) & ~kn)
        rays = [j for j in range(8) if pat >> j & 1]
        k = hits[rays][:, ys, xs].T                                       # [P][n]
        off = k[:, :, None] * dirs[rays][None, :, :]
        zs = z[ys[:, None] + off[:, :, 0], xs[:, None] + off[:, :, 1]]
        assert kn[ys[:, None] + off[:, :, 0], xs[:, None] + off[:, :, 1]].all()
        s = bordered(off, zs, vg, cellsize)
        out[ys, xs], var[ys, xs] = s["est"], np.maximum(s["var"], 0.0)
        eb[ys, xs] = 0.5 * ulp32(s["est"]) + 64 * EPS * s["cond"] * s["absw_z"]
        vb[ys, xs] = 0.5 * ulp32(var[ys, xs]) + 64 * EPS * s["cond"] * s["absw_g"]
    rays = ~kn & (pattern != 0)
    near = np.zeros((H, W), bool)
    if idx is not None:
        near = ~kn & ~rays & (idx >= 0)
        out[near] = z.ravel()[idx[near]]
        g = vg.gamma(np.float64(cellsize) * np.sqrt(np.asarray(d2)[near].astype(np.float64)))
        var[near] = 2.0 * g
        vb[near] = 0.5 * ulp32(var[near]) + 64 * EPS * 2.0 * g
    return {"out": out, "var": var, "est_bound": eb, "var_bound": vb, "nhits": have.sum(0),
            "counts": [int(rays.sum()), int(near.sum()), int((~kn & ~rays & ~near).sum())]}
