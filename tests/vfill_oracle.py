"""numpy oracle of the harmonic void fill (mvp_gan/src/fill_voids.py, csrc/voidfill.hip): every unknown pixel p solves
sum_{q in N4(p) inside the raster} (u_q - u_p) = 0 with u = z on the known pixels, solved per 4-connected component of the
unknowns as a dense fp64 system.  numpy only (the GPU machine may lack scipy)."""
from collections import deque

import numpy as np

MAX_COMPONENT = 4500          # dense solve per component: keep them small


def known_mask(z, mask=None, nodata=None):
    k = np.isfinite(z)
    if mask is not None:
        k &= np.asarray(mask) != 0
    if nodata is not None and not np.isnan(nodata):
        k &= z != np.float32(nodata)
    return k


def _neighbours(i, H, W):
    y, x = divmod(i, W)
    if y > 0:
        yield i - W
    if y < H - 1:
        yield i + W
    if x > 0:
        yield i - 1
    if x < W - 1:
        yield i + 1


def components(unknown):
    """4-connected components of the unknown pixels: a list of int64 arrays of flat indices (ascending)."""
    H, W = unknown.shape
    flat = unknown.ravel()
    seen = np.zeros(flat.size, bool)
    out = []
    for s in np.flatnonzero(flat):
        if seen[s]:
            continue
        seen[s] = True
        comp, q = [], deque([int(s)])
        while q:
            i = q.popleft()
            comp.append(i)
            for j in _neighbours(i, H, W):
                if flat[j] and not seen[j]:
                    seen[j] = True
                    q.append(j)
        out.append(np.array(sorted(comp), np.int64))
    return out


def solve(z, known, max_component=MAX_COMPONENT):
    """fp64 fill: known pixels as z, unknowns solved per component; all NaN when nothing is known."""
    z = np.asarray(z)
    H, W = z.shape
    u = np.where(known, z.astype(np.float64), np.nan)
    if not known.any():
        return u
    zf = z.astype(np.float64).ravel()
    kf = known.ravel()
    uf = u.ravel()
    for comp in components(~known):
        n = comp.size
        if n > max_component:
            raise ValueError(f"vfill_oracle: a component of {n} unknowns, more than {max_component}")
        pos = {int(i): j for j, i in enumerate(comp)}
        A = np.zeros((n, n))
        b = np.zeros(n)
        for j, i in enumerate(comp):
            for q in _neighbours(int(i), H, W):
                A[j, j] += 1.0
                if kf[q]:
                    b[j] += zf[q]
                else:
                    A[j, pos[q]] -= 1.0
        uf[comp] = np.linalg.solve(A, b)
    return uf.reshape(H, W)


def residual(u, known):
    """sum_{q in N4(p) inside} (u_q - u_p) at every unknown pixel (0 at known pixels), fp64."""
    u = np.asarray(u, np.float64)
    r = np.zeros_like(u)
    r[1:, :] += u[:-1, :] - u[1:, :]
    r[:-1, :] += u[1:, :] - u[:-1, :]
    r[:, 1:] += u[:, :-1] - u[:, 1:]
    r[:, :-1] += u[:, 1:] - u[:, :-1]
    return np.where(known, 0.0, r)


def harmonic_field(H, W, coef, x0=0.0, y0=0.0, scale=1.0):
    """a + b x + c y + d (x^2 - y^2) + e x y + f (x^3 - 3 x y^2) at x = (col - x0) / scale, y = (row - y0) / scale: satisfies
    the 5-point equation exactly at every interior pixel (fp64)."""
    a, b, c, d, e, f = coef
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x = (x - x0) / scale
    y = (y - y0) / scale
    return a + b * x + c * y + d * (x * x - y * y) + e * x * y + f * (x ** 3 - 3 * x * y * y)


def disc(H, W, cy, cx, r):
    y, x = np.mgrid[0:H, 0:W]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r
