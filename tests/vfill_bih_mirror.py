"""numpy mirror of the biharmonic void fill (fill_voids(method="biharmonic"), csrc/voidfill.hip): the
operator A = D(D(.)) restricted to the unknowns, the inner right-hand-side conjugate gradients around the V-cycle of
tests/vfill_pcg_mirror.py (G, an approximate solve of -D(e) = f), and the outer flexible conjugate gradients preconditioned by
M r = G(G(r)).  Vectors are held in the kernels' storage types: the outer x, D(x), the residual and every dot product fp64,
the direction p, the preconditioner's input and output and the whole inner solve fp32.  dt_in = float64 turns the inner solve
to fp64 as well: a tight reference solve.  numpy only."""
import math

import numpy as np

from tests import vfill_pcg_mirror as M


def apply_A(x, known):
    """D(D(x)) at the unknowns (0 at the known pixels); x carries whatever the known pixels hold, fp64."""
    out = M.diff_sum(M.diff_sum(np.asarray(x, np.float64)))
    out[np.asarray(known, bool)] = 0
    return out


def _dot(a, b):
    return float(np.dot(np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()))


def inner_solve(plan, f, known, inner, counter=None):
    """G(f): `inner` iterations of flexible PCG on -D(e) = f over the unknowns (e = 0 at the known pixels) from e = 0, the
    V-cycle as the preconditioner; inner = 1 is one bare cycle.  Every vector has the plan's type; the dots are fp64.
    -> e; counter [cycles, restarts] is advanced."""
    dt = plan.dt
    counter = [0, 0] if counter is None else counter
    zero = np.zeros(known.shape, dt)
    f = f.astype(dt)
    z = M.vcycle(plan, zero, f)
    counter[0] += 1
    if inner == 1:
        return z
    e, r, p = zero.copy(), f, z.copy()
    rho = _dot(r, z)
    for k in range(1, inner + 1):
        ap = -M.diff_sum(p)
        ap[known] = 0
        pap = _dot(p, ap)
        alpha = dt(0)
        if rho != 0.0:
            a = dt(rho / pap) if pap > 0 else dt(np.nan)
            if np.isfinite(a):
                alpha = a
            else:
                counter[1] += 1
        e = M._fma(alpha, p, e) if plan.fma else e + alpha * p
        if k == inner:
            break
        r = M.diff_sum(e, f)
        r[known] = 0
        rz_old = _dot(r, z)
        z = M.vcycle(plan, zero, r)
        counter[0] += 1
        rho_new = _dot(r, z)
        beta = dt(0)
        if rho != 0.0:
            b = dt((rho_new - rz_old) / rho)
            if np.isfinite(b):
                beta = b
            else:
                counter[1] += 1
        p = M._fma(beta, p, z) if plan.fma else z + beta * p
        rho = rho_new
    return e


def solve(z, known, tol=None, max_cycles=200, inner=3, dt_in=np.float32, trace=None, fma=False):
    """The outer loop.  -> (raster in dt_in, info: cycles (outer iterations), vcycles, change, tol, converged, restarts,
    history).
    trace: a dict whose "states" list receives the outer loop's state as tg_vfill_bih_start (entry 0) and the k-th
    tg_vfill_bih_iter (entry k) leave it in the block at sc_out and in xa, r, z and the current p: the launches and so the timing
    of the scalars are those of the pcg loop (the docstring of tests/vfill_pcg_mirror.py; z' = G(G(r')) takes the cycle's
    place), x and r are fp64, and an entry is recorded once the next pass has formed pap and alpha: run max_cycles = k + 1 to
    see the state after k iterations (trace["stop"] = n ends the loop once n entries are there).  With trace=None the result is
    bit for bit what it was.  fma: the compiled kernels' rounding of the fp32 updates (vfill_pcg_mirror.Plan)."""
    known = np.asarray(known, bool)
    plan = M.Plan(known, dt_in, fma)
    v, c, rng = M._start(z, known, np.float32)                 # the set-up is fp32 whatever the solve's type
    t = 1e-6 * rng if tol is None else tol
    x = v.astype(np.float64)
    cnt = [0, 0]
    cycles, change, conv, restarts, hist = 0, 0.0, True, 0, []

    def pre(r):
        return inner_solve(plan, inner_solve(plan, r.astype(dt_in), known, inner, cnt), known, inner, cnt)

    if not known.all():
        conv = False
        r = -apply_A(x, known)
        zz = pre(r)
        p = zz.copy()
        rho = _dot(r, zz)
        rz_old, beta = 0.0, np.float32(0)
        while cycles < max_cycles:
            pap = _dot(p, apply_A(p, known))
            cycles += 1
            if trace is not None:
                M._record(trace, np.float32, x=x, r=r, z=zz, p=p, rho=rho, pap=pap, rz_old=rz_old, beta=beta)
                if len(trace["states"]) == trace.get("stop"):   # the caller wants no more entries: skip the rest of the pass
                    break
            if rho == 0.0:
                change = 0.0
                conv = True
                break
            alpha = np.float32(rho / pap) if pap > 0 else np.float32(np.nan)
            if not np.isfinite(alpha):
                restarts += 1
                p = zz.copy()
                hist.append(math.inf)
                continue
            d = np.float64(alpha) * p.astype(np.float64)
            x = x + d
            change = float(np.abs(d)[~known].max())
            hist.append(change)
            if change <= t:
                conv = True
                break
            r = -apply_A(x, known)
            rz_old = _dot(r, zz)
            zz = pre(r)
            rho_new = _dot(r, zz)
            beta = np.float32((rho_new - rz_old) / rho)
            if not np.isfinite(beta):
                restarts += 1
                beta = np.float32(0)
            p = M._fma(beta, p, zz) if plan.fma else (zz + dt_in(beta) * p).astype(dt_in)
            rho = rho_new
    out = M._finish(z, known, x.astype(dt_in), dt_in(c))
    return out, {"cycles": cycles, "vcycles": cnt[0], "change": change, "tol": t, "converged": conv,
                 "restarts": restarts + cnt[1], "history": hist}


def solve64(z, known, tol=0.0, max_cycles=200, inner=3):
    """The tight solve: every vector fp64."""
    return solve(z, known, tol=tol, max_cycles=max_cycles, inner=inner, dt_in=np.float64)


# ---- the scenes of DESIGN.md section 8q -----------------------------------------------------------------------------
def field(H, W):
    """The smooth closed-form terrain of section 8q's table (fp64)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.sin(x / 17.0) * np.cos(y / 23.0) + 0.3 * np.sin(x / 5.0 + y / 7.0)


def case(name):
    """-> (z float32, known) of a named scene."""
    from tests import vfill_bih_oracle as BO
    from tests import vfill_oracle as VO
    if name == "37x53 disc, cubic":
        return BO.bih_poly_raster(37, 53).astype(np.float32), ~VO.disc(37, 53, 18, 26, 9)
    if name == "128x160 void [30:93, 61:130], cubic":
        return BO.bih_poly_raster(128, 160).astype(np.float32), M.box_known(128, 160, [(30, 93, 61, 130)])
    if name == "300x300 void [64:192, 128:256], cubic":
        return BO.bih_poly_raster(300, 300).astype(np.float32), M.box_known(300, 300, [(64, 192, 128, 256)])
    if name == "128x160 void [30:93, 61:130]":
        return field(128, 160).astype(np.float32), M.box_known(128, 160, [(30, 93, 61, 130)])
    if name == "300x300 void [64:192, 128:256]":
        return field(300, 300).astype(np.float32), M.box_known(300, 300, [(64, 192, 128, 256)])
    if name == "96x80 left half":
        return field(96, 80).astype(np.float32), M.box_known(96, 80, [(0, 96, 0, 40)])
    assert name == "257x129 1% known", name
    return field(257, 129).astype(np.float32), np.random.default_rng(3).random((257, 129)) < 0.01


def terrain(H, W, seed):
    """Smooth relief plus a little noise on an offset, float32."""
    rng = np.random.default_rng(seed)
    return (100.0 + 20.0 * field(H, W) + rng.normal(0, 0.05, (H, W))).astype(np.float32)


def small_scene(name):
    """-> (z float32, mask or None, nodata or None) of the scenes checked against the dense oracle (at most 4000 unknowns)."""
    from tests import vfill_oracle as VO
    H, W = (int(v) for v in name.split()[0].split("x"))
    z = terrain(H, W, H * 1000 + W)
    k = np.ones((H, W), bool)
    what = name.split(None, 1)[1]
    if what == "hole":
        k[H // 5:H - H // 4, W // 4:W - W // 5] = False
    elif what == "disc":
        k = ~VO.disc(H, W, H // 2, W // 2, 10)
    elif what == "corner past the tile":
        k[20:, 50:] = False
    elif what == "four-tile corner":
        k[28:40, 58:72] = False
    elif what == "ring in a tile without unknowns":
        k[10:20, 60:64] = False
    elif what == "edges and a corner":
        k[0:8, 10:20] = False                                  # on the top edge
        k[20:30, 1:9] = False                                  # one pixel from the left edge
        k[40:, 70:] = False                                    # the bottom right corner
    elif what == "left half":
        k[:, :W // 2] = False
    elif what == "runs":
        n = max(H, W)
        r = np.ones(n, bool)
        r[: n // 20] = False
        r[n // 3: n // 3 + n // 4] = False
        r[n - 7:] = False
        r[n // 2 + 50::97] = False
        k = r.reshape(H, W)
    elif what == "one known":
        k[:] = False
        k[3, 4] = True
    elif what == "all known":
        pass
    elif what == "nothing known":
        k[:] = False
    elif what == "3% known":
        k = np.random.default_rng(5).random((H, W)) < 0.03
    else:
        assert what == "nan inf nodata mask", name
        z[5:9, 6:11] = np.nan
        z[20, 30:34] = np.inf
        z[21, 30:34] = -np.inf
        z[30:36, 40:47] = -9999.0
        k[12:18, 20:31] = False
        return z, k.astype(np.float32), -9999.0
    return z, k.astype(np.float32), None


SMALL_SCENES = ("1x1 all known", "5x7 hole", "16x16 hole", "32x64 disc", "33x65 corner past the tile", "70x140 four-tile corner",
                "40x130 ring in a tile without unknowns", "48x80 edges and a corner", "96x80 left half", "1x300 runs",
                "300x1 runs", "12x9 one known", "20x30 all known", "20x30 nothing known", "40x50 nan inf nodata mask",
                "48x64 3% known")
