"""CPU oracle of the depression fill (csrc/depfill.hip, mvp_gan/src/fill_depressions.py), numpy + heapq.

Known pixels: mask != 0, finite, != nodata.  Connectivity 8 or 4.  An outlet is a known pixel on the raster's edge or with an
unknown neighbour of that connectivity.  W(p) = min over connected paths of known pixels from p to an outlet of the max of z
along the path; unknown pixels are NaN.  Two independent forms: a priority-flood (Barnes, Lehman, Mulla 2014, Algorithm 1, no
epsilon) and the synchronous relaxation W <- max(z, min(W, min over the neighbours W)) from W = z at outlets, +inf elsewhere.
Values stay float32 throughout; only comparisons are made, so both are exact."""
import heapq
import math

import numpy as np

N4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
N8 = N4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


def neighbours(conn):
    if conn not in (4, 8):
        raise ValueError(f"connectivity {conn!r} must be 8 or 4")
    return N8 if conn == 8 else N4


def known_map(z, mask=None, nodata=None):
    z = np.asarray(z, np.float32)
    k = np.isfinite(z)
    if mask is not None:
        k &= np.asarray(mask) != 0
    if nodata is not None and not math.isnan(nodata):
        k &= z != np.float32(nodata)
    return k


def outlets(known, conn=8):
    """Known pixels on the edge or with an unknown neighbour."""
    H, W = known.shape
    pad = np.zeros((H + 2, W + 2), bool)                       # outside the raster counts as unknown: the edge is an outlet
    pad[1:-1, 1:-1] = known
    out = np.zeros((H, W), bool)
    for dy, dx in neighbours(conn):
        out |= ~pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    return out & known


def priority_flood(z, known, conn=8):
    """-> W float32 [H][W], NaN at unknown pixels, +inf at known pixels no outlet reaches (there are none: every component of
    known pixels has a pixel on the edge or next to an unknown one)."""
    z = np.asarray(z, np.float32)
    H, W = z.shape
    out = np.full((H, W), np.nan, np.float32)
    out[known] = np.inf
    done = np.zeros((H, W), bool)
    heap = []
    for y, x in zip(*np.nonzero(outlets(known, conn))):
        heap.append((float(z[y, x]), int(y), int(x)))
        done[y, x] = True
        out[y, x] = z[y, x]
    heapq.heapify(heap)
    nb = neighbours(conn)
    while heap:
        lvl, y, x = heapq.heappop(heap)
        for dy, dx in nb:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and known[yy, xx] and not done[yy, xx]:
                done[yy, xx] = True
                v = max(float(z[yy, xx]), lvl)                  # both are float32 values: the max is one of them
                out[yy, xx] = np.float32(v)
                heapq.heappush(heap, (v, yy, xx))
    return out


def relax_start(z, known, conn=8):
    z = np.asarray(z, np.float32)
    w = np.full(z.shape, np.nan, np.float32)
    w[known] = np.inf
    o = outlets(known, conn)
    w[o] = z[o]
    return w


def relax_step(z, w, known, conn=8):
    """One synchronous step on a state with NaN at unknown pixels."""
    H, W = z.shape
    pad = np.full((H + 2, W + 2), np.inf, np.float32)
    pad[1:-1, 1:-1] = np.where(known, w, np.float32(np.inf))
    m = pad[1:-1, 1:-1].copy()
    for dy, dx in neighbours(conn):
        m = np.minimum(m, pad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
    out = w.copy()
    out[known] = np.maximum(z[known], m[known])
    return out


def relax(z, known, conn=8, max_steps=None):
    """The synchronous relaxation to its fixed point (or max_steps steps) -> (W, steps taken)."""
    z = np.asarray(z, np.float32)
    w = relax_start(z, known, conn)
    steps = 0
    while max_steps is None or steps < max_steps:
        nw = relax_step(z, w, known, conn)
        steps += 1
        if np.array_equal(nw.view(np.uint32), w.view(np.uint32)):
            break
        w = nw
    return w, steps


def finish(z, w, known):
    """-> (out, depth, flags) as tg_depfill_finish defines them."""
    z = np.asarray(z, np.float32)
    out = np.full(z.shape, np.nan, np.float32)
    depth = np.full(z.shape, np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        raised = known & (w > z)
        reached = known & np.isfinite(w)
    keep = known & ~raised
    out[keep] = z[keep]
    depth[keep] = 0
    up = raised & reached
    out[up] = w[up]
    depth[up] = w[up] - z[up]
    return out, depth, raised.astype(np.uint8)


def stats(z, w, known, sel=None):
    """-> {raised, unreached, counted, depth_sum (fp64, correctly rounded: math.fsum), max_depth (exact)} over the known pixels,
    with sel those with sel != 0."""
    z = np.asarray(z, np.float32)
    k = known.copy()
    if sel is not None:
        k &= np.asarray(sel) != 0
    with np.errstate(invalid="ignore"):
        raised = k & (w > z)
    unreached = raised & np.isinf(w)
    fin = raised & ~unreached
    d = w[fin].astype(np.float64) - z[fin].astype(np.float64)
    return {"raised": int(raised.sum()), "unreached": int(unreached.sum()), "counted": int(k.sum()),
            "depth_sum": math.fsum(d.tolist()), "max_depth": float(d.max()) if d.size else 0.0}


def depressions(flags):
    """8-connected components of flags != 0 (scipy)."""
    from scipy import ndimage
    return int(ndimage.label(np.asarray(flags) != 0, structure=np.ones((3, 3), int))[1])


# ---- scenes ---------------------------------------------------------------------------------------------------------------
def spiral_wall(n=130, pitch=4):
    """A 4-connected rectangular spiral wall, one pixel thick, inside the border ring of an n x n raster: it starts at (pitch, 1),
    next to the ring, runs east and turns right whenever the pixel `pitch` ahead is the ring or wall."""
    wall = np.zeros((n, n), bool)
    free = np.zeros((n, n), bool)
    free[1:n - 1, 1:n - 1] = True
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    r, c, d, turns = pitch, 1, 0, 0
    wall[r, c] = True
    while turns < 2:
        dr, dc = dirs[d]
        ok = free[r + dr, c + dc] and not wall[r + dr, c + dc]
        for k in range(1, pitch + 1):
            ar, ac = r + dr * k, c + dc * k
            if not (0 <= ar < n and 0 <= ac < n) or not free[ar, ac] or wall[ar, ac]:
                ok = False
                break
        if ok:
            r, c, turns = r + dr, c + dc, 0
            wall[r, c] = True
        else:
            d, turns = (d + 1) % 4, turns + 1
    return wall


def spiral_scene(n=130, pitch=4):
    """-> (z float32 [n][n], channel bool [n][n]).  The wall is at 1100 m; the channel floor descends towards the centre,
    990 + 0.1 * Chebyshev distance to the centre; the border ring is at 1050 m with one lower cell (1040 m) at (pitch, 0), which
    touches the wall's first pixel by an edge and the channel only by its corners.  So with connectivity 4 every channel pixel
    is raised to 1050 m, with 8 to 1040 m, and the path that decides it runs the whole channel, across every tile seam."""
    wall = spiral_wall(n, pitch)
    y, x = np.mgrid[0:n, 0:n]
    c = (n - 1) / 2.0
    r = np.maximum(np.abs(y - c), np.abs(x - c))
    z = (990.0 + 0.1 * r).astype(np.float32)
    z[wall] = 1100.0
    ring = np.ones((n, n), bool)
    ring[1:n - 1, 1:n - 1] = False
    z[ring] = 1050.0
    z[pitch, 0] = 1040.0
    return z, ~wall & ~ring


def pits_scene(H, W, seed, npits=20, base=1000.0, relief=3.0):
    """Random relief near `base` with npits dug pits (1 to 9 px wide, 2 to 6 m deep)."""
    rng = np.random.default_rng(seed)
    z = (base + rng.normal(0, relief, (H, W))).astype(np.float32)
    for _ in range(npits):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        z[y:y + h, x:x + w] -= np.float32(rng.uniform(2, 6))
    return z


def gap_scene(n=9, lo=2, hi=6):
    """Ground at 980 m that drains to the edge, a square wall ring (rows and columns lo..hi) at 1020 m around a basin at 990 m,
    and the wall's corner (lo, lo) dug to 985 m: a one-pixel diagonal gap.  With connectivity 8 the basin drains through it and
    nothing is raised; with 4 the basin is raised to the wall, 1020 m."""
    z = np.full((n, n), 980.0, np.float32)
    z[lo:hi + 1, lo:hi + 1] = 1020.0
    z[lo + 1:hi, lo + 1:hi] = 990.0
    z[lo, lo] = 985.0
    return z


def bowl(z, cy, cx, radius, floor, slope):
    """Carve a round bowl into z: floor + slope * distance to (cy, cx) within `radius`, strictly rising from its centre."""
    y, x = np.mgrid[0:z.shape[0], 0:z.shape[1]]
    r = np.hypot(y - cy, x - cx)
    out = z.copy()
    out[r <= radius] = (floor + slope * r[r <= radius]).astype(np.float32)
    return out
