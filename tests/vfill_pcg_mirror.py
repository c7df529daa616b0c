"""numpy mirror of the masked multigrid V-cycle of csrc/voidfill.hip and of the flexible conjugate-gradient loop around it
(fill_voids(solver="pcg")).  Values are held in `dt` (fp32 as on the GPU; fp64 gives a tight reference
solve), dot products are accumulated in fp64.  The passes of the kernels are tile-independent, so the mirror runs every sweep
on the whole level at once.  numpy only.

Traces (tests/vfill_trace.py compares them with what the kernels leave in their workspaces).  vcycle(..., trace={}) fills
trace["f"], trace["down"] and trace["up"], one entry per level: the restricted right-hand side (None at level 0 of the plain
cycle), the field after the down sweeps (None on the coarsest level, which has no down pass) and the field after the
prolongation and the up sweeps, or after the coarsest solve.  solve_pcg(..., trace={}) appends to trace["states"] the state as
tg_vfill_pcg_start (entry 0) and the k-th tg_vfill_pcg_iter (entry k) leave it.  One call launches, in this order: the step
x' = x + alpha p and r' = b - A x' with the partials of r'.z (the old z); the cycle z' = M r'; the partials of r'.z'; the beta
scalar kernel (rz_old, rz_new, beta = (rz_new - rz_old) / rho with the rho of the call before, then rho = rz_new); the
direction p' = z' + beta p into the other p buffer with the partials of p'.Ap'; the alpha scalar kernel (pap, alpha = rho / pap,
restart, parity ^= 1).  So after call k the block holds x_k, r_k, z_k, p_k, rho = rz_new = r_k.z_k, rz_old = r_k.z_{k-1},
beta_k, pap = p_k.Ap_k and the alpha that the NEXT call's step applies; parity names the buffer that holds p_k (1 after the
start).  The loop below forms pap and alpha at the top of the next pass, so an entry is recorded there: to see the state after
k iterations run max_cycles = k + 1.  With trace=None nothing is recorded and every result is bit for bit what it was."""
import math

import numpy as np

CMAX = 16


def levels(H, W):
    out = [(int(H), int(W))]
    while max(out[-1]) > CMAX:
        h, w = out[-1]
        out.append(((h + 1) // 2, (w + 1) // 2))
    return out


def _fma(a, b, c):
    """a * b + c rounded once, as the fused multiply-add that the compiler forms on the GPU: the product of two fp32 numbers is
    exact in fp64, and the second rounding of the sum (fp64, then fp32) moves the result only at an exact tie of the first."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


class Plan:
    """Per level: fixed flags (any fixed child), neighbour counts and the two colour masks of the unknown cells.
    fma (fp32 only): round as the compiled kernels do where the compiler contracts a product and a sum into one fused
    multiply-add, which the source does not show: the first sum of the prolongation (9 a + 3 b becomes fma(3, b, 9 a)) and the
    SOR update u + omega q of the coarsest level; solve_pcg and vfill_bih_mirror add their x + alpha p and z + beta p.  The
    stage tests of DESIGN.md section 8af compare the kernels with this variant; the default is the source's arithmetic."""

    def __init__(self, known, dt=np.float32, fma=False):
        self.dt = dt
        self.fma = bool(fma) and dt == np.float32
        fix = np.asarray(known, bool)
        self.lv = []
        for l, (h, w) in enumerate(levels(*fix.shape)):
            if l:
                pad = np.zeros((2 * h, 2 * w), bool)
                pad[:fix.shape[0], :fix.shape[1]] = fix
                fix = _coarse_fix(pad)
            n = np.zeros((h, w), dt)
            n[1:, :] += 1
            n[:-1, :] += 1
            n[:, 1:] += 1
            n[:, :-1] += 1
            yy, xx = np.mgrid[0:h, 0:w]
            free = ~fix & (n > 0)
            self.lv.append({"H": h, "W": w, "fix": fix, "n": np.maximum(n, 1).astype(dt), "fma": self.fma,
                            "col": [free & (((yy + xx) & 1) == c) for c in (0, 1)]})

    @property
    def L(self):
        return len(self.lv)


def _coarse_fix(pad):
    """The fixed cells of the next level from the zero-padded fixed map: any fixed child."""
    return pad[0::2, 0::2] | pad[0::2, 1::2] | pad[1::2, 0::2] | pad[1::2, 1::2]


def diff_sum(u, f=None):
    """f_p + sum_{q in N4(p) inside} (u_q - u_p), the neighbours in the kernels' order: up, down, left, right."""
    acc = np.zeros_like(u) if f is None else f.copy()
    acc[1:, :] += u[:-1, :] - u[1:, :]
    acc[:-1, :] += u[1:, :] - u[:-1, :]
    acc[:, 1:] += u[:, :-1] - u[:, 1:]
    acc[:, :-1] += u[:, 1:] - u[:, :-1]
    return acc


def _half_sweep(u, f, lv, col, omega=None):
    acc = diff_sum(u, f) / lv["n"]
    m = lv["col"][col]
    if omega is not None and lv["fma"]:
        u[m] = _fma(omega, acc, u)[m]
        return
    if omega is not None:
        acc = omega * acc
    u[m] = (u + acc)[m]


def _sweeps(u, f, lv, count=2):
    for _ in range(count):
        _half_sweep(u, f, lv, 0)
        _half_sweep(u, f, lv, 1)


def _restrict(r, lv, nx):
    h, w = nx["H"], nx["W"]
    pad = np.zeros((2 * h, 2 * w), r.dtype)
    pad[:r.shape[0], :r.shape[1]] = r
    f = (pad[0::2, 0::2] + pad[0::2, 1::2]) + (pad[1::2, 0::2] + pad[1::2, 1::2])
    if lv["H"] == 1 or lv["W"] == 1:
        f = f * r.dtype.type(2)
    f[nx["fix"]] = 0
    return f


def _prolong(e, lv):
    H, W = lv["H"], lv["W"]
    hn, wn = e.shape
    y, x = np.arange(H), np.arange(W)
    Y, X = y >> 1, x >> 1
    ny = np.clip(Y + np.where(y & 1, 1, -1), 0, hn - 1)
    nx = np.clip(X + np.where(x & 1, 1, -1), 0, wn - 1)
    t = e.dtype.type
    if lv["fma"]:
        out = (_fma(t(3), e[np.ix_(ny, X)], t(9) * e[np.ix_(Y, X)]) + t(3) * e[np.ix_(Y, nx)] + e[np.ix_(ny, nx)]) * t(0.0625)
    else:
        out = (t(9) * e[np.ix_(Y, X)] + t(3) * e[np.ix_(ny, X)] + t(3) * e[np.ix_(Y, nx)] + e[np.ix_(ny, nx)]) * t(0.0625)
    out[lv["fix"]] = 0
    return out


def _coarsest(u, f, lv):
    n = max(lv["H"], lv["W"])
    om = u.dtype.type(np.float32(2.0 / (1.0 + math.sin(math.pi / (2.0 * n + 1.0)))))
    for _ in range(8 * n + 16):
        _half_sweep(u, f, lv, 0, om)
        _half_sweep(u, f, lv, 1, om)


DOWN_SWEEPS = UP_SWEEPS = 2


def vcycle(plan, u0, f0=None, trace=None):
    """One V-cycle from u0 at level 0 (known values in place, or 0 with a right-hand side f0); -> the new level-0 values.
    trace: a dict that receives per level f, down and up (the module docstring)."""
    dt = plan.dt
    lv = plan.lv
    u = [None] * plan.L
    f = [None] * plan.L
    down = [None] * plan.L
    u[0] = u0.copy()
    f[0] = f0
    for l in range(plan.L - 1):
        if l:
            u[l] = np.zeros((lv[l]["H"], lv[l]["W"]), dt)
        _sweeps(u[l], f[l], lv[l], DOWN_SWEEPS)
        if trace is not None:
            down[l] = u[l].copy()
        r = diff_sum(u[l], f[l])
        r[lv[l]["fix"]] = 0
        f[l + 1] = _restrict(r, lv[l], lv[l + 1])
    l = plan.L - 1
    if l:
        u[l] = np.zeros((lv[l]["H"], lv[l]["W"]), dt)
    _coarsest(u[l], f[l], lv[l])
    for l in range(plan.L - 2, -1, -1):
        u[l] = u[l] + _prolong(u[l + 1], lv[l])
        _sweeps(u[l], f[l], lv[l], UP_SWEEPS)
    if trace is not None:
        trace["f"] = [None if a is None else a.copy() for a in f]
        trace["down"] = down
        trace["up"] = [a.copy() for a in u]
    return u[0]


def _start(z, known, dt):
    known = np.asarray(known, bool)
    zk = np.asarray(z)[known].astype(dt)
    lo, hi = zk.min(), zk.max()
    c = dt(lo * dt(0.5) + hi * dt(0.5))
    v = np.zeros(known.shape, dt)
    v[known] = zk - c
    return v, c, float(hi) - float(lo)


def _finish(z, known, v, c):
    out = (v + c).astype(v.dtype)
    out[known] = np.asarray(z)[known].astype(v.dtype)
    return out


def solve_mg(z, known, tol=None, max_cycles=50, dt=np.float32):
    """The plain solver: V-cycles until the largest change over the unknowns is <= tol.  -> (raster, info)."""
    known = np.asarray(known, bool)
    plan = Plan(known, dt)
    v, c, rng = _start(z, known, dt)
    t = 1e-6 * rng if tol is None else tol
    cycles, change, conv, hist = 0, 0.0, True, []
    if not known.all():
        conv = False
        while cycles < max_cycles:
            w = vcycle(plan, v)
            change = float(np.abs(w - v)[~known].max())
            hist.append(change)
            v = w
            cycles += 1
            if change <= t:
                conv = True
                break
    return _finish(z, known, v, c), {"cycles": cycles, "change": change, "tol": t, "converged": conv, "history": hist}


def _dot(a, b):
    return float(np.dot(a.astype(np.float64).ravel(), b.astype(np.float64).ravel()))


def _neg_lap(p, known):
    """A p: the masked graph Laplacian of a direction (p is 0 at the known pixels)."""
    ap = -diff_sum(p)
    ap[known] = 0
    return ap


def _beta_num(rz_new, rz_old):
    """The numerator of the flexible (Polak-Ribiere) beta."""
    return rz_new - rz_old


def _record(trace, dt, **kw):
    """One entry of trace["states"]: the scalars as the alpha kernel leaves them (alpha 0 with the restart flag when rho / pap
    is no usable step, alpha 0 without it at rho = 0), the vectors copied."""
    rho, pap = kw["rho"], kw["pap"]
    alpha, restart = dt(0), 0
    if rho != 0.0:
        with np.errstate(all="ignore"):
            a = dt(rho / pap) if pap > 0 else dt(np.nan)
        if np.isfinite(a):
            alpha = a
        else:
            restart = 1
    st = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
    st.update(alpha=alpha, restart=restart, rz_new=rho, parity=(len(trace.setdefault("states", [])) + 1) & 1)
    trace["states"].append(st)


def solve_pcg(z, known, tol=None, max_cycles=50, dt=np.float32, trace=None, fma=False):
    """Flexible conjugate gradients preconditioned by one V-cycle; one iteration = one cycle.  -> (raster, info).
    trace: a dict whose "states" list receives the state after the start and after each iteration (the module docstring); with
    trace["stop"] = n the loop ends once n entries are there.  fma: the compiled kernels' rounding (Plan)."""
    known = np.asarray(known, bool)
    plan = Plan(known, dt, fma)
    x, c, rng = _start(z, known, dt)
    t = 1e-6 * rng if tol is None else tol
    zero = np.zeros(known.shape, dt)
    cycles, change, conv, restarts, hist = 0, 0.0, True, 0, []

    def resid(x):
        r = diff_sum(x)
        r[known] = 0
        return r

    if not known.all():
        conv = False
        r = resid(x)
        zz = vcycle(plan, zero, r)
        p = zz.copy()
        rho = _dot(r, zz)
        rz_old, beta = 0.0, dt(0)
        while cycles < max_cycles:
            ap = _neg_lap(p, known)
            pap = _dot(p, ap)
            cycles += 1
            if trace is not None:
                _record(trace, dt, x=x, r=r, z=zz, p=p, rho=rho, pap=pap, rz_old=rz_old, beta=beta)
                if len(trace["states"]) == trace.get("stop"):   # the caller wants no more entries: skip the rest of the pass
                    break
            if rho == 0.0:
                change = 0.0
                conv = True
                break
            alpha = dt(rho / pap) if pap > 0 else dt(np.nan)
            if not np.isfinite(alpha):
                restarts += 1                                   # x is left alone; the direction starts again from z
                p = zz.copy()
                hist.append(math.inf)
                continue
            d = alpha * p
            x = _fma(alpha, p, x) if plan.fma else x + d
            change = float(np.abs(d)[~known].max())
            hist.append(change)
            if change <= t:
                conv = True
                break
            r = resid(x)
            rz_old = _dot(r, zz)
            zz = vcycle(plan, zero, r)
            rho_new = _dot(r, zz)
            beta = dt(_beta_num(rho_new, rz_old) / rho)
            if not np.isfinite(beta):
                restarts += 1
                beta = dt(0)
            p = _fma(beta, p, zz) if plan.fma else zz + beta * p
            rho = rho_new
    return _finish(z, known, x, c), {"cycles": cycles, "change": change, "tol": t, "converged": conv, "restarts": restarts,
                                      "history": hist}


# ---- the cases of DESIGN.md section 8n ----------------------------------------------------------------------------------
def field(H, W):
    """A smooth closed-form terrain (fp64) for the aligned-void cases."""
    from tests import vfill_oracle as VO
    return VO.harmonic_field(H, W, (120, 4, -3, 2, 1, 0.2), W / 2, H / 2, max(H, W) / 2)


def border_field(H, W, side, coef):
    """coef[0] + sum_k coef[k] cos(k pi (y + 1/2) / H) (l^s + l^-s) / 2 with l + 1 / l = 4 - 2 cos(k pi / H) and s the distance
    to the raster's `side` ("left" or "right") edge plus 1/2: satisfies the 5-point equation with the natural border rule at
    every pixel, the top and bottom rows and the `side` column included (its mirror images across those edges are itself), so
    it is the exact fill of voids that touch them (fp64).  vfill_oracle.harmonic_field holds only off the border."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    s = x + 0.5 if side == "left" else W - 0.5 - x
    out = np.full((H, W), float(coef[0]))
    for k, c in enumerate(coef[1:], 1):
        th = math.pi * k / H
        lam = math.acosh(2.0 - math.cos(th))
        out += c * np.cos(th * (y + 0.5)) * np.cosh(lam * s)
    return out


def box_known(H, W, boxes):
    k = np.ones((H, W), bool)
    for y0, y1, x0, x1 in boxes:
        k[y0:y1, x0:x1] = False
    return k


# the voids of "512x512 left half" touch the left, top and bottom edges, those of "768x768 missing tiles" the top and right
BORDER_SIDE = {"512x512 left half": "left", "768x768 missing tiles": "right"}

ALIGNED = {
    "300x300 void [64:192, 128:256]": (300, 300, [(64, 192, 128, 256)]),
    "512x512 void [128:384, 128:384]": (512, 512, [(128, 384, 128, 384)]),
    "512x512 left half": (512, 512, [(0, 512, 0, 256)]),
    "768x768 missing tiles": (768, 768, [(256, 512, 256, 512), (0, 128, 512, 768)]),
}
