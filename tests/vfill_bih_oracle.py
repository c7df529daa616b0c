"""Dense fp64 oracle of the biharmonic void fill (fill_voids(method="biharmonic")).  With L the masked
5-point graph Laplacian of the raster (natural border: a neighbour outside the raster is no neighbour), U the unknown pixels and
K the known ones, the fill minimises |L u|^2 over u_U with u_K = z_K.  Only the rows S = U and its 4-neighbours depend on u_U,
so with B = L[S, U] and B_K = L[S, K] the normal equations are  B^T B x = -B^T B_K z_K.  numpy only."""
import numpy as np

MAX_UNKNOWN = 4000


def laplacian_rows(known):
    """-> (S indices, B [|S|, |U|], Bk as a function z -> B_K z_K) for the flat raster."""
    known = np.asarray(known, bool)
    H, W = known.shape
    unk = np.flatnonzero(~known.ravel())
    assert 0 < unk.size <= MAX_UNKNOWN, unk.size
    col = -np.ones(H * W, np.int64)
    col[unk] = np.arange(unk.size)
    inS = np.zeros(H * W, bool)
    inS[unk] = True
    y, x = np.divmod(unk, W)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        yy, xx = y + dy, x + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        inS[yy[ok] * W + xx[ok]] = True
    S = np.flatnonzero(inS)
    return S, unk, col


def solve(z, known):
    """-> fp64 raster: z at the known pixels, the biharmonic fill elsewhere.  K must not be empty."""
    known = np.asarray(known, bool)
    H, W = known.shape
    out = np.asarray(z, np.float64).copy()
    out[~known] = 0.0
    if known.all():
        return out
    assert known.any()
    S, unk, col = laplacian_rows(known)
    B = np.zeros((S.size, unk.size))
    g = np.zeros(S.size)                                   # B_K z_K
    flat = out.ravel()
    kf = known.ravel()
    sy, sx = np.divmod(S, W)
    for r, (p, y, x) in enumerate(zip(S, sy, sx)):
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy, x + dx
            if not (0 <= yy < H and 0 <= xx < W):
                continue
            q = yy * W + xx
            # row p of L: sum_q (u_q - u_p)
            if kf[q]:
                g[r] += flat[q]
            else:
                B[r, col[q]] += 1.0
            if kf[p]:
                g[r] -= flat[p]
            else:
                B[r, col[p]] -= 1.0
    xs = np.linalg.solve(B.T @ B, -(B.T @ g))
    flat[unk] = xs
    return out


def energy_gradient(u, known):
    """D(D(u)) at the unknowns: 0 at the solution."""
    from tests.vfill_pcg_mirror import diff_sum
    r = diff_sum(diff_sum(np.asarray(u, np.float64)))
    r[np.asarray(known, bool)] = 0
    return r


def bih_poly(y, x, H, W):
    """A fixed polynomial with D(D(f)) = 0 off the border that is far from harmonic: with X, Y the coordinates from the raster's
    centre in units of half its longer side, D(f) = (0.8 X + 4) / s^2, linear, so D(D(f)) = 0 exactly.  The Y^2 term carries
    most of the range, which is what a harmonic fill cannot follow."""
    s = max(H, W) / 2.0
    X, Y = (np.asarray(x, np.float64) - W / 2) / s, (np.asarray(y, np.float64) - H / 2) / s
    return 100.0 * (0.3 * X ** 3 - 0.5 * Y ** 2 * X + 0.8 * X * Y + 2.0 * Y ** 2 + 0.5 * X)


def bih_poly_raster(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return bih_poly(y, x, H, W)
