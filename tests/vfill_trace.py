"""Stage-by-stage comparison of the void-fill solvers with their numpy mirrors: one comparator, the
walks over the stages of a V-cycle trace and of a conjugate-gradient state in the order in which the kernels produce them, and
the cases.  A trace comes from tests/vfill_pcg_mirror.py or tests/vfill_bih_mirror.py, or is read from the kernels' workspaces
(tests/test_hip_vfill_stages.py).  The first failing stage localises the fault.  numpy only."""
import re

import numpy as np

from tests import vfill_pcg_mirror as M

EPS32 = 2.0 ** -23
# bound = K x max(max |ref32 - ref64|, EPS32 x scale).  K: the next power of two above twice the worst deviation of the GPU from
# the fp64 mirror in that unit, measured over every case and stage (the table of DESIGN.md section 8af).
K_FIELD = 4.0
K_SCALAR = 4.0


class StageError(AssertionError):
    """A stage outside its bound; .stage is its name, .over the deviation in units of the bound (inf for an exact stage)."""

    def __init__(self, stage, msg, over=float("inf")):
        super().__init__(msg)
        self.stage = stage
        self.over = over


def _level(stage):
    m = re.search(r"/L(\d+)/", stage + "/")
    return int(m.group(1)) if m else None


def compare(stage_name, got, ref64, ref32, scale=None, K=None, log=None):
    """-> (deviation max |got - ref64|, bound K x max(max |ref32 - ref64|, EPS32 x scale)); scale: max |ref64| when None; K:
    K_FIELD for arrays and K_SCALAR for scalars when None.  Raises StageError with the stage's name, its level and the worst
    element's coordinates when the deviation is above the bound or not a number.  log: a list that receives (stage, deviation,
    unit) with unit = bound / K."""
    g = np.asarray(got, np.float64)
    a = np.asarray(ref64, np.float64)
    b = np.asarray(ref32, np.float64)
    if g.shape != a.shape or b.shape != a.shape:
        raise StageError(stage_name, f"{stage_name}: shapes {g.shape}, {a.shape}, {b.shape} differ")
    if K is None:
        K = K_FIELD if a.ndim else K_SCALAR
    if scale is None:
        scale = float(np.abs(a).max()) if a.size else 0.0
    unit = max(float(np.abs(b - a).max()) if a.size else 0.0, EPS32 * float(scale))
    bound = K * unit if unit > 0 else 0.0              # both mirrors exactly 0 (a right-hand side under fixed cells): so is `got`
    d = np.abs(g - a)
    dev = float(d.max()) if d.size else 0.0
    if log is not None:
        log.append((stage_name, dev, unit))
    if not dev <= bound:
        bad = np.where(np.isnan(d), np.inf, d)
        at = tuple(int(i) for i in np.unravel_index(int(np.argmax(bad)), d.shape)) if d.ndim else ()
        raise StageError(stage_name, f"stage {stage_name} (level {_level(stage_name)}): deviation {dev:.3e} > bound {bound:.3e} "
                         f"(K {K:g} x unit {unit:.3e}, scale {scale:.3e}); worst at {at}: got {g[at]!r}, fp64 mirror {a[at]!r}, "
                         f"fp32 mirror {b[at]!r}", over=dev / bound if bound > 0 else float("inf"))
    return dev, bound


def exact(stage_name, got, ref):
    """Bit-for-bit (or integer) equality of a stage that has no rounding: flags, counts, parity."""
    g, r = np.asarray(got), np.asarray(ref)
    if g.shape != r.shape or not np.array_equal(g, r):
        at = ()
        if g.shape == r.shape and g.ndim:
            at = tuple(int(i) for i in np.argwhere(g != r)[0])
        raise StageError(stage_name, f"stage {stage_name} (level {_level(stage_name)}): not equal, first at {at}")


# ---- the stages of one V-cycle, in the order of the launches ------------------------------------------------------------
def cycle_stages(L):
    """[(key, level)]: down 0, f 1, down 1, ..., f L-1, up L-1 (the coarsest solve), up L-2, ..., up 0."""
    out = []
    for l in range(L - 1):
        out += [("down", l), ("f", l + 1)]
    return out + [("up", l) for l in range(L - 1, -1, -1)]


def compare_cycle(prefix, got, ref64, ref32, K=None, log=None):
    """Every stage of a vcycle trace (dicts f, down, up of per-level arrays).  An entry that the mirror does not have (f of level 0
    in the plain cycle, down of the coarsest level) must be None in `got` as well.  -> [(stage, deviation, bound)]."""
    L = len(ref64["up"])
    out = []
    for key, l in cycle_stages(L):
        name = f"{prefix}/L{l}/{key}"
        if ref64[key][l] is None:
            if got[key][l] is not None:
                raise StageError(name, f"stage {name}: the mirror has nothing to compare here")
            continue
        out.append((name,) + compare(name, got[key][l], ref64[key][l], ref32[key][l], K=K, log=log))
    if ref64["f"][0] is not None:
        name = f"{prefix}/L0/f"
        out.append((name,) + compare(name, got["f"][0], ref64["f"][0], ref32["f"][0], K=K, log=log))
    return out


def compare_plan(got_fix, plan):
    """The fixed flags of every level, exactly."""
    for l, lv in enumerate(plan.lv):
        exact(f"setup/L{l}/fix", got_fix[l], lv["fix"])


# ---- the state of the conjugate gradients after the start and after each iteration ---------------------------------------
# Per state, in the order in which a call produces them.  "x" ... "alpha" are compared with the mirrors.  The stages with a dot
# in their name check the scalars against the state's OWN vectors and scalars, which needs no mirror: "rz_old.dot", "rz_new.dot"
# and "pap.dot" are the fp64 dot products of the vectors that were read (within DOT_TOL x sum |a_i b_i|: the order of an fp64
# sum), "rho.same", "beta.formula" and "alpha.formula" the scalar kernels' arithmetic, which numpy repeats bit for bit.
STATE_ORDER = ("x", "r", "rz_old.dot", "rz_old", "z", "rz_new.dot", "rz_new", "rho.same", "rho", "beta.formula", "beta", "p",
               "pap.dot", "pap", "alpha.formula", "alpha")
SCALARS = ("rz_old", "rz_new", "rho", "beta", "pap", "alpha")
# A scalar on which the fp32 and the fp64 mirror disagree by more than GATE of its size has no reference: it is rounding of a
# cancelling sum (r'.z of the old z at iteration 1, which the step makes 0 in exact arithmetic; every scalar once the residual
# is rounding itself, from iteration 1 on where the preconditioner is exact), and a quotient of two such numbers (alpha, beta)
# is not even bounded by the mirrors' spread.  Such a stage is not compared with the mirrors; it is still pinned, more sharply
# than a bound could, by the dotted stages above.  The gated stages are returned, and the tests assert which they are.
# alpha = rho / pap and beta = (rz_new - rz_old) / rho are gated with their numerators and with pap as well: the quotient of
# numbers without a reference has none, even where the two mirrors happen to agree on it (both near 1 for a converged solve).
GATE = 2.0 ** -10
DERIVED = {"alpha": ("rho", "pap"), "beta": ("rz_new",)}
DOT_TOL = 2.0 ** -32              # 2 n 2^-53 for n <= 2^20 terms: two orders of summing the same exact products


# The gated stages of the pcg loop (start and 3 iterations), per case; both test files assert them.  r'.z of the old z is
# rounding at iteration 1 everywhere, and on two cases later as well.  Where the preconditioner is exact (one level; the
# checkerboard, whose unknowns have known neighbours only) the first step solves the system, the residual is rounding from
# iteration 1 on, and so is every scalar formed from it.
_NOISE = frozenset(f"pcg/iter{k}/{q}" for k in (1, 2, 3) for q in SCALARS)
PCG_GATED = {"70x135": {"pcg/iter1/rz_old"}, "33x65": {"pcg/iter1/rz_old", "pcg/iter3/rz_old"}, "1x300": {"pcg/iter1/rz_old"},
             "300x1": {"pcg/iter1/rz_old"}, "3x131500": {"pcg/iter1/rz_old", "pcg/iter2/rz_old", "pcg/iter3/rz_old"},
             "5x7": _NOISE, "16x16": _NOISE, "37x53 checkerboard": _NOISE}


def neg_lap(p, known):
    """A p of the Laplace solvers: the masked graph Laplacian, in p's type and the kernels' order of sums."""
    ap = -M.diff_sum(p)
    ap[np.asarray(known, bool)] = 0
    return ap


def _f32(expr):
    with np.errstate(all="ignore"):
        return np.float32(expr())


def _own(name, g, prev, apply, dot_tol):
    """The dotted stage `name` of state g (prev: the state before it, or None)."""
    key, kind = name.rsplit("/", 1)[1].split(".")
    if kind == "dot":
        a, b = {"rz_old": lambda: (g["r"], prev["z"] if prev else np.zeros_like(g["z"])), "rz_new": lambda: (g["r"], g["z"]),
                "pap": lambda: (g["p"], apply(g["p"]))}[key]()
        t = np.asarray(a, np.float64).ravel() * np.asarray(b, np.float64).ravel()
        ref, tol = float(t.sum()), dot_tol * float(np.abs(t).sum())
        dev = abs(float(g[key]) - ref)
        if not dev <= tol:
            raise StageError(name, f"stage {name}: {g[key]!r} is not the dot product of the state's own vectors {ref!r} "
                             f"(off by {dev:.3e}, allowed {tol:.3e})", over=dev / tol if tol > 0 else float("inf"))
        return
    if key == "rho":
        want, have = float(g["rz_new"]), float(g["rho"])
    elif key == "beta":
        want = np.float32(0)
        if prev is not None and not prev["restart"] and float(prev["rho"]) != 0.0:
            bf = _f32(lambda: (np.float64(g["rz_new"]) - np.float64(g["rz_old"])) / np.float64(prev["rho"]))
            want = bf if np.isfinite(bf) else want
        have = np.float32(g["beta"])
    else:
        want = np.float32(0)
        if float(g["rho"]) != 0.0:
            af = _f32(lambda: np.float64(g["rho"]) / np.float64(g["pap"]))
            want = af if float(g["pap"]) > 0 and np.isfinite(af) else want
        have = np.float32(g["alpha"])
    if not have == want:
        raise StageError(name, f"stage {name}: {have!r} is not what the state's own scalars give, {want!r}")


def compare_states(prefix, got, ref64, ref32, apply, K_field=None, K_scalar=None, log=None, gated=None, dot_tol=DOT_TOL):
    """got, ref64, ref32: lists of states (dicts as vfill_pcg_mirror._record writes them), entry 0 the start; apply: p -> A p.
    The stages of STATE_ORDER per state, then restart and parity exactly.  Scalars are compared relative to their own size.
    gated: a list that receives the names of the scalar stages that have no reference (GATE).  -> [(stage, deviation, bound)]."""
    out = []
    for k, (g, a, b) in enumerate(zip(got, ref64, ref32)):
        step = f"{prefix}/" + ("start" if k == 0 else f"iter{k}")
        for key in STATE_ORDER:
            name = f"{step}/{key}"
            if "." in key:
                _own(name, g, got[k - 1] if k else None, apply, dot_tol)
                continue
            if key in SCALARS and any(abs(float(b[q]) - float(a[q])) > GATE * abs(float(a[q]))
                                      for q in (key,) + DERIVED.get(key, ())):
                if gated is not None:
                    gated.append(name)
                continue
            K = K_scalar if key in SCALARS else K_field
            out.append((name,) + compare(name, g[key], a[key], b[key], K=K, log=log))
        for key in ("restart", "parity"):
            exact(f"{step}/{key}", int(g[key]), int(a[key]))
            exact(f"{step}/{key}", int(b[key]), int(a[key]))
    if not len(got) == len(ref64) == len(ref32):
        raise StageError(prefix, f"{prefix}: {len(got)}, {len(ref64)}, {len(ref32)} states")
    return out


def tile_sums(a, ty=32, tx=64):
    """The sum of a [H][W] over each ty x tx tile, fp64, -> [tiles_y][tiles_x]."""
    a = np.asarray(a, np.float64)
    H, W = a.shape
    ny, nx = -(-H // ty), -(-W // tx)
    pad = np.zeros((ny * ty, nx * tx))
    pad[:H, :W] = a
    return pad.reshape(ny, ty, nx, tx).sum(axis=(1, 3))


def tiles_with_unknown(known, ty=32, tx=64):
    """[tiles_y][tiles_x] bool: the tile holds a pixel that is not known (fixed)."""
    return tile_sums(~np.asarray(known, bool), ty, tx) > 0


def cell_tile_mask(active, H, W, ty=32, tx=64):
    """[H][W] bool: the cell lies in a tile of `active`."""
    return np.repeat(np.repeat(active, ty, axis=0), tx, axis=1)[:H, :W]


# ---- the cases ------------------------------------------------------------------------------------------------------------
def terrain(H, W, seed, noise=0.3):
    """The terrain of tests/test_hip_fill_voids_pcg.py."""
    from tests import vfill_oracle as VO
    rng = np.random.default_rng(seed)
    f = VO.harmonic_field(H, W, (120, 4, -3, 2, 1, 0.2), W / 2, H / 2, max(H, W) / 2)
    return (f + 6 * np.sin(np.arange(W) / 17.0)[None, :] * np.cos(np.arange(H) / 23.0)[:, None]
            + rng.normal(0, noise, (H, W))).astype(np.float32)


def _runs(H, W):
    n = max(H, W)
    k = np.ones(n, bool)
    k[: n // 20] = False                               # touches the first end: its first unknown has one neighbour
    k[n // 3: n // 3 + n // 4] = False                 # interior run
    k[n - 7:] = False                                  # touches the other end
    k[n // 2 + 50::97] = False                         # single pixels
    return k.reshape(H, W)


def case(name):
    """-> (z float32 [H][W], known bool [H][W]) of a named case; the shapes are the smallest that reach each path."""
    if name == "70x135":
        # 5 levels (35x68, 18x34, 9x17, 5x9), 3 x 3 tiles at level 0 and 2 x 2 at level 1, H or W odd at four levels
        H, W = 70, 135
        k = np.ones((H, W), bool)
        k[16:48, 30:100] = False                       # a 32 x 70 box across the four-tile corner at (32, 64); it holds whole
        #                                                16 x 16 blocks, so the coarsest level has free cells
        k[31, 2:27] = False                            # 1-px stroke along the last row of the first tile row
        k[2:15, 64] = False                            # 1-px stroke along the first column of the second tile column
        k[0:3, 0:4] = False                            # the raster's top left corner
        k[66:70, 131:135] = False                      # the bottom right corner, in the partial last tile row and column
        k[65:68, 70:80] = False                        # inside the partial last tile row
        k[50:55, 129:133] = False                      # inside the partial last tile column
        act = tiles_with_unknown(k)
        assert not act[2, 0] and not act[0, 2] and act[1, 0] and act[2, 1], act     # a halo reads a tile without unknowns
        return terrain(H, W, 21), k
    if name == "33x65":
        k = np.ones((33, 65), bool)
        k[20:33, 50:65] = False                        # covers the corner pixel (32, 64), the only one of its tile
        return terrain(33, 65, 22), k
    if name == "5x7":
        k = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 1, 1, 1], [1, 0, 0, 0, 0, 1, 1], [1, 1, 0, 0, 1, 1, 0],
                      [1, 1, 1, 1, 1, 0, 0]], bool)
        return terrain(5, 7, 0), k
    if name == "16x16":
        from tests import vfill_oracle as VO
        return terrain(16, 16, 1), ~VO.disc(16, 16, 9, 6, 5)
    if name in ("1x300", "300x1"):
        H, W = (int(v) for v in name.split("x"))
        return terrain(H, W, 1), _runs(H, W)
    if name == "3x131500":
        # 2055 level-0 tiles (> the grid limit 2048: the tile loop's second trip), heights 3 -> 2 -> 1: rscale 1, then 2
        H, W = 3, 131500
        k = np.ones((H, W), bool)
        cols = np.arange(7, W, 40)
        k[(cols // 40) % 3, cols] = False              # one pixel every 40 columns: every 64-column tile holds an unknown
        k[:, 500:530] = False
        k[0:2, 70000:70100] = False
        k[1, 131200:131500] = False                    # a run in the tiles with an id >= 2048, to the raster's end
        k[:, 131080:131090] = False
        assert tiles_with_unknown(k).all()
        return terrain(H, W, 23), k
    assert name == "37x53 checkerboard", name
    yy, xx = np.mgrid[0:37, 0:53]
    return terrain(37, 53, 2), (yy + xx) % 2 == 0      # every unknown's neighbours are known: every coarse cell is fixed


CASES = ("70x135", "33x65", "5x7", "16x16", "1x300", "300x1", "3x131500", "37x53 checkerboard")


# ---- the mirrors' traces, computed once per case --------------------------------------------------------------------------
def cycle_refs(known, u_in, f_in=None):
    """One V-cycle of the fp64 and the fp32 mirror from the same start -> (trace64, trace32).  Here and below the fp32 mirror
    rounds as the compiled kernels do (fma=True, vfill_pcg_mirror.Plan)."""
    out = []
    for dt in (np.float64, np.float32):
        tr = {}
        M.vcycle(M.Plan(known, dt, fma=True), np.asarray(u_in, dt), None if f_in is None else np.asarray(f_in, dt), trace=tr)
        out.append(tr)
    return out


def pcg_refs(z, known, iters):
    """-> (states64, states32) of solve_pcg: the start and `iters` iterations."""
    out = []
    for dt in (np.float64, np.float32):
        tr = {"stop": iters + 1}
        M.solve_pcg(z, known, tol=0.0, max_cycles=iters + 1, dt=dt, trace=tr, fma=True)
        out.append(tr["states"])
    return out


def bih_refs(z, known, iters, inner):
    from tests import vfill_bih_mirror as B
    out = []
    for dt in (np.float64, np.float32):
        tr = {"stop": iters + 1}
        B.solve(z, known, tol=0.0, max_cycles=iters + 1, inner=inner, dt_in=dt, trace=tr, fma=True)
        out.append(tr["states"])
    return out
