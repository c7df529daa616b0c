"""CPU oracle of the multiple-flow-direction accumulation, the slope and the wetness index (csrc/mfd.hip,
mvp_gan/src/flow_routing.py), numpy only.

Inputs are a routing of tests/flow_oracle.py: the routed surface w (float32), known, the D8 direction grid.  Neighbour k = 0..7
is code k + 1 (E, SE, S, SW, W, NW, N, NE).

Fractions of a known pixel q.  For j = 0..7 with neighbour n_j inside the raster and known: d_j = w[q] - w[n_j], one float32
subtract, valid iff d_j > 0 (a NaN never is); t_j = float64(d_j) raised to the integer exponent e by e - 1 float64 multiplies
t = t * d, times cdiag = 2 ** (-(e + 1) / 2) for odd j (a diagonal); S = the float64 sum of the valid t_j in the order j = 0..7.
S > 0 ("dispersive"): f_j = t_j / S.  Otherwise, with direction[q] in 1..8 ("single"): f = 1.0 to the D8 receiver.  Otherwise
(OUT, PIT, unknown; a "sink"): nothing.

Accumulation.  A[p] = 1.0 for a known p; then for k = 0..7 in order, if neighbour n_k gives to p (its fraction in direction
(k + 4) % 8 is > 0): A[p] = A[p] + f * A[n_k], a float64 multiply and a float64 add.  0 at unknown pixels.  Two independent
forms: Kahn's topological order with in-degree counts (accumulate_kahn) and a level-synchronous relaxation that recomputes,
from gathered values, every pixel whose donors are all final (accumulate_relax).

Slope: Horn's 3x3 stencil in float32 (slope).  Wetness: ln(a / max(slope, min_slope)) with a = float32(A) * float32(cellsize);
the GPU's logf is compared against the float64 logarithm of the float32 operands (twi_ref)."""
from collections import deque

import numpy as np

from tests import flow_oracle as FO

DY, DX = FO.DY, FO.DX
DISPERSIVE, SINGLE, SINK = 1, 2, 3


def cdiag(e):
    return 2.0 ** (-(e + 1) / 2)


def check_exponent(e):
    import numbers
    if isinstance(e, (bool, np.bool_)) or not isinstance(e, numbers.Integral) or not 1 <= e <= 8:
        raise ValueError(f"exponent {e!r} must be an integer in [1, 8]")
    return int(e)


def fractions(w, known, direction, e, cd=None):
    """-> (F float64 [8][H][W]: F[j][q] the fraction q gives to its neighbour j; S float64 [H][W]; cls uint8 [H][W]: 0 unknown,
    DISPERSIVE, SINGLE, SINK)."""
    e = check_exponent(e)
    cd = cdiag(e) if cd is None else cd
    w = np.asarray(w, np.float32)
    known = np.asarray(known, bool)
    H, W = w.shape
    T = np.zeros((8, H, W), np.float64)
    ok = np.zeros((8, H, W), bool)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for j in range(8):
            d = (w - FO._shift(w, DY[j], DX[j], np.float32(np.nan))).astype(np.float32)
            ok[j] = known & FO._shift(known, DY[j], DX[j], False) & (d > 0)
            d64 = d.astype(np.float64)
            t = d64.copy()
            for _ in range(e - 1):
                t = t * d64
            if j & 1:
                t = t * cd
            T[j] = np.where(ok[j], t, 0.0)
        S = np.zeros((H, W), np.float64)
        for j in range(8):
            S = S + T[j]                                           # + 0.0 where the term is not valid: the same bits
        disp = known & (S > 0)
        F = np.zeros((8, H, W), np.float64)
        for j in range(8):
            F[j] = np.where(disp & ok[j], T[j] / np.where(disp, S, 1.0), 0.0)
    code = np.asarray(direction).astype(np.int64)
    single = known & ~disp & (code >= 1) & (code <= 8)
    for j in range(8):
        F[j][single & (code == j + 1)] = 1.0
    cls = np.zeros((H, W), np.uint8)
    cls[known] = SINK
    cls[single] = SINGLE
    cls[disp] = DISPERSIVE
    return F, S, cls


def donor_fractions(F):
    """G[k][p] = the fraction neighbour k of p gives to p (0 where it gives nothing or lies outside)."""
    return np.stack([FO._shift(F[(k + 4) % 8], DY[k], DX[k], 0.0) for k in range(8)])


def _padded(F, known):
    H, W = known.shape
    Wp = W + 2
    pad = lambda a, fill: np.pad(a, 1, constant_values=fill).ravel()
    G = donor_fractions(F)
    off = [DY[k] * Wp + DX[k] for k in range(8)]
    inner = (np.arange(1, H + 1)[:, None] * Wp + np.arange(1, W + 1)[None, :]).ravel()
    return [pad(G[k], 0.0) for k in range(8)], [pad(F[j], 0.0) for j in range(8)], pad(known, False), off, inner


def accumulate_kahn(F, known):
    """-> (A float64 [H][W], the longest path in steps, pixels visited)."""
    known = np.asarray(known, bool)
    H, W = known.shape
    Gp, Fp, kp, off, inner = _padded(F, known)
    G = [g.tolist() for g in Gp]
    Fl = [f.tolist() for f in Fp]
    indeg = np.zeros(kp.size, np.int64)
    for k in range(8):
        indeg += Gp[k] > 0
    indeg = indeg.tolist()
    A = [0.0] * kp.size
    length = [0] * kp.size
    q = deque(int(p) for p in inner[kp[inner]] if indeg[p] == 0)
    seen = 0
    while q:
        p = q.popleft()
        seen += 1
        a = 1.0
        for k in range(8):
            g = G[k][p]
            if g > 0:
                a = a + g * A[p + off[k]]
        A[p] = a
        for j in range(8):
            if Fl[j][p] > 0:
                r = p + off[j]
                if length[p] + 1 > length[r]:
                    length[r] = length[p] + 1
                indeg[r] -= 1
                if indeg[r] == 0:
                    q.append(r)
    out = np.array(A, np.float64)[inner].reshape(H, W)
    return out, max(length) if length else 0, seen


def accumulate_relax(F, known):
    """The level-synchronous form: in a round every pixel that is not final and whose donors are all final is computed, all from
    the values before the round -> (A float64 [H][W], rounds; pixels left at -1.0 would sit on a cycle)."""
    known = np.asarray(known, bool)
    H, W = known.shape
    Gp, Fp, kp, off, inner = _padded(F, known)
    A = np.where(kp, -1.0, 0.0)
    cand = inner[kp[inner]]
    rounds = 0
    while cand.size:
        cand = cand[A[cand] < 0]
        ok = np.ones(cand.size, bool)
        for k in range(8):
            ok &= ~(Gp[k][cand] > 0) | (A[cand + off[k]] >= 0)
        ready = cand[ok]
        if not ready.size:
            break
        new = np.ones(ready.size, np.float64)
        for k in range(8):
            g = Gp[k][ready]
            new = np.where(g > 0, new + g * A[ready + off[k]], new)
        A[ready] = new
        rounds += 1
        cand = np.unique(np.concatenate([(ready + off[j])[Fp[j][ready] > 0] for j in range(8)]))
    return A[inner].reshape(H, W), rounds


def mass_out(A, cls):
    """The sum of A over the sinks (math.fsum: the exact sum rounded once)."""
    import math
    return math.fsum(A[cls == SINK].tolist())


def counts(cls):
    return {"dispersive": int((cls == DISPERSIVE).sum()), "single": int((cls == SINGLE).sum()), "sinks": int((cls == SINK).sum())}


def mfd(w, known, direction, e):
    """-> dict(A float64, acc float32, cls, counts, longest, max, mass_out) by Kahn's order; asserts that it visits every known
    pixel."""
    F, S, cls = fractions(w, known, direction, e)
    A, longest, seen = accumulate_kahn(F, known)
    assert seen == int(np.asarray(known, bool).sum()), "the MFD graph has a cycle"
    return {"A": A, "acc": A.astype(np.float32), "cls": cls, "S": S, "F": F, "counts": counts(cls), "longest": longest,
            "max": float(A.max()), "mass_out": mass_out(A, cls)}


def route_mfd(z, mask=None, nodata=None, fill=True, e=1):
    """flow_oracle.route, then mfd on its surface -> (routing dict, mfd dict)."""
    r = FO.route(z, mask, nodata, fill)
    return r, mfd(r["w"], r["known"], r["dir"], e)


# ---- slope and wetness ----------------------------------------------------------------------------------------------------
def slope(w, known, cellsize=1.0):
    """Horn's tan(beta) in float32: a b c / d . f / g h i with rows top to bottom, a neighbour outside the raster or unknown
    replaced by the centre; gx = ((c - a) + 2 (f - d)) + (i - g), gy = ((g - a) + 2 (h - b)) + (i - c),
    sqrt(gx gx + gy gy) / float32(8 cellsize); NaN at unknown pixels."""
    w = np.asarray(w, np.float32)
    known = np.asarray(known, bool)

    def nb(dy, dx):
        return np.where(FO._shift(known, dy, dx, False), FO._shift(w, dy, dx, np.float32(0)), w).astype(np.float32)
    a, b, c = nb(-1, -1), nb(-1, 0), nb(-1, 1)
    d, f = nb(0, -1), nb(0, 1)
    g, h, i = nb(1, -1), nb(1, 0), nb(1, 1)
    two = np.float32(2)
    with np.errstate(invalid="ignore", over="ignore"):
        gx = ((c - a) + two * (f - d)) + (i - g)
        gy = ((g - a) + two * (h - b)) + (i - c)
        s = np.sqrt(gx * gx + gy * gy) / np.float32(8.0 * cellsize)
    assert s.dtype == np.float32
    return np.where(known, s, np.float32(np.nan)).astype(np.float32)


def twi_ref(acc, slp, known, cellsize=1.0, min_slope=1e-3):
    """ln in float64 of the float32 operands: a = float32(acc) * float32(cellsize), the slope not below float32(min_slope) (fmax:
    a NaN slope counts as min_slope); NaN at unknown pixels -> float64 [H][W]."""
    a = (np.asarray(acc, np.float32) * np.float32(cellsize)).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.fmax(np.asarray(slp, np.float32), np.float32(min_slope))
        t = np.log(a.astype(np.float64) / s.astype(np.float64))
    return np.where(np.asarray(known, bool), t, np.nan)


def twi_bound(ref):
    """|twi - ref| allowed: 2^-21 + 2^-22 |ref| (three ulp of the ratio from slope and divide, logf at 1 ulp and the rounding)."""
    return 2.0 ** -21 + 2.0 ** -22 * np.abs(ref)


def wetness_stats(sel, twi_t, twi_p):
    """-> (cells, sum d, sum |d|, sum d * d in float64 (math.fsum), max |d| as float32) of d = float32(twi_p - twi_t) where sel and
    both are finite."""
    import math
    t, p = np.asarray(twi_t, np.float32), np.asarray(twi_p, np.float32)
    use = (np.asarray(sel) != 0) & np.isfinite(t) & np.isfinite(p)
    d = (p[use] - t[use]).astype(np.float32).astype(np.float64)
    return (int(use.sum()), math.fsum(d.tolist()), math.fsum(np.abs(d).tolist()), math.fsum((d * d).tolist()),
            np.float32(np.abs(d).max()) if d.size else np.float32(0))


# ---- scenes -----------------------------------------------------------------------------------------------------------------
EXPONENTS = (1, 4, 8)
NODATA = -9999.0


def void_scene():
    """96x70 of rounded relief with a 20x20 void (NaN) and one nodata pixel on the border -> z."""
    z = FO.rounded_pits(96, 70, 11, npits=8)
    z[40:60, 25:45] = np.nan
    z[0, 33] = NODATA
    return z


def scenes():
    """name -> (z, nodata, fill): the scenes of tests/flow_oracle.py the MFD tests run, every one at EXPONENTS."""
    from tests import depfill_oracle as DO
    return {"pits": (DO.pits_scene(130, 130, 3), None, True),
            "rounded": (FO.rounded_pits(130, 130, 7), None, True),
            "spiral": (FO.spiral_flat()[0], None, False),
            "serpentine": (FO.serpentine()[0], None, False),
            "lake": (FO.lake_scene()[0], None, False),
            "void": (void_scene(), NODATA, True),
            "unfilled": (FO.rounded_pits(70, 90, 5, npits=10), None, False)}


_CACHE = {}


def scene_ref(name, e):
    """(z, nodata, fill, routing, mfd dict) of a named scene at exponent e, computed once and left unchanged."""
    if (name, "route") not in _CACHE:
        z, nodata, fill = scenes()[name]
        r = FO.route(z, None, nodata, fill)
        for v in list(r.values()) + [z]:
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[(name, "route")] = (z, nodata, fill, r)
    z, nodata, fill, r = _CACHE[(name, "route")]
    if (name, e) not in _CACHE:
        m = mfd(r["w"], r["known"], r["dir"], e)
        for v in m.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[(name, e)] = m
    return z, nodata, fill, r, _CACHE[(name, e)]
