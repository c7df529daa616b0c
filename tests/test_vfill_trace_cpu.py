"""CPU checks of the stage comparison of the void-fill solvers (tests/vfill_trace.py), the fp32 mirror
standing in for the GPU: the unmutated mirror passes every stage with K = 1; every mutant of the cycle and of the conjugate
gradients fails, at the stage where it first shows, by at least 10 x the bound that the GPU test uses (K_FIELD, K_SCALAR); the
assertions of the GPU suites on the converged result pass most of the mutants (the table of section 8af); tracing leaves the
mirrors' results bit for bit."""
import contextlib

import numpy as np
import pytest

from tests import vfill_bih_mirror as B
from tests import vfill_pcg_mirror as M
from tests import vfill_trace as T

MARGIN = 10.0


# ---- the mutants: each patches one function of the mirror ---------------------------------------------------------------
def _prolong_const(z, known):
    def f(e, lv):
        out = e[np.ix_(np.arange(lv["H"]) >> 1, np.arange(lv["W"]) >> 1)].copy()
        out[lv["fix"]] = 0
        return out
    return {"_prolong": f}


def _restrict_three(z, known):
    def f(r, lv, nx):
        h, w = nx["H"], nx["W"]
        pad = np.zeros((2 * h, 2 * w), r.dtype)
        pad[:r.shape[0], :r.shape[1]] = r
        # the child (0, 0) is lost.  It has the colour of the first half-sweep; the residual of the other colour, (0, 1) and
        # (1, 0), is rounding after the last half-sweep, so losing one of those moves nothing
        pad[0::2, 0::2] = 0
        out = (pad[0::2, 0::2] + pad[0::2, 1::2]) + (pad[1::2, 0::2] + pad[1::2, 1::2])
        if lv["H"] == 1 or lv["W"] == 1:
            out = out * r.dtype.type(2)
        out[nx["fix"]] = 0
        return out
    return {"_restrict": f}


def _no_doubling(z, known):
    def f(r, lv, nx):
        h, w = nx["H"], nx["W"]
        pad = np.zeros((2 * h, 2 * w), r.dtype)
        pad[:r.shape[0], :r.shape[1]] = r
        out = (pad[0::2, 0::2] + pad[0::2, 1::2]) + (pad[1::2, 0::2] + pad[1::2, 1::2])
        out[nx["fix"]] = 0
        return out
    return {"_restrict": f}


def _coarsest_plain(z, known):
    return {"_coarsest": lambda u, f, lv: M._sweeps(u, f, lv, 2)}


def _band(z, known):
    """The level-0 correction lost in 8 columns (rows on a one-column raster) through the middle of the unknowns."""
    H, W = known.shape
    ax = 1 if W > 1 else 0
    c = int(np.median(np.nonzero(~known)[ax]))
    lo = max(0, min(c - 4, known.shape[ax] - 8))
    orig = M._prolong

    def f(e, lv):
        out = orig(e, lv)
        if (lv["H"], lv["W"]) == (H, W):
            if ax:
                out[:, lo:lo + 8] = 0
            else:
                out[lo:lo + 8, :] = 0
        return out
    return {"_prolong": f}


def _one_up_sweep(z, known):
    return {"UP_SWEEPS": 1}


def _all_children(z, known):
    def f(pad):
        return pad[0::2, 0::2] & pad[0::2, 1::2] & pad[1::2, 0::2] & pad[1::2, 1::2]
    return {"_coarse_fix": f}


def _dot_drops_block(z, known):
    """Every dot product loses the 32 x 64 tile that holds the most unknowns."""
    n = T.tile_sums(~known)
    ty, tx = np.unravel_index(int(np.argmax(n)), n.shape)

    def f(a, b):
        p = a.astype(np.float64) * b.astype(np.float64)
        p[32 * ty:32 * ty + 32, 64 * tx:64 * tx + 64] = 0
        return float(p.ravel().sum())
    return {"_dot": f}


def _fletcher_reeves(z, known):
    return {"_beta_num": lambda rz_new, rz_old: rz_new}


def _p_not_zeroed(z, known):
    """A p from a direction that holds 1 at the fixed cells."""
    def f(p, known_):
        q = p.copy()
        q[known_] = 1
        ap = -M.diff_sum(q)
        ap[known_] = 0
        return ap
    return {"_neg_lap": f}


MUTANTS = {
    "prolongation piecewise constant": _prolong_const,
    "restriction drops a child": _restrict_three,
    "no x2 on a level one cell high or wide": _no_doubling,
    "coarsest level: 2 plain sweeps": _coarsest_plain,
    "correction lost in a band": _band,
    "one sweep on the up pass": _one_up_sweep,
    "all children fixed": _all_children,
    "pcg: a block dropped from the dots": _dot_drops_block,
    "pcg: Fletcher-Reeves beta": _fletcher_reeves,
    "pcg: p not zeroed at the fixed cells": _p_not_zeroed,
}


@contextlib.contextmanager
def mutant(name, z, known):
    patch = MUTANTS[name](z, known) if name else {}
    old = {k: getattr(M, k) for k in patch}
    try:
        for k, v in patch.items():
            setattr(M, k, v)
        yield
    finally:
        for k, v in old.items():
            setattr(M, k, v)


# ---- the walk the GPU test makes, on mirrors ----------------------------------------------------------------------------
_REFS = {}


def _refs(name):
    """The unmutated mirrors of a case, computed once: plan, start, one cycle and the pcg states in fp64 and fp32."""
    if name not in _REFS:
        z, k = T.case(name)
        v = M._start(z, k, np.float32)[0]
        _REFS[name] = (z, k, v, M.Plan(k, np.float32), T.cycle_refs(k, v), T.pcg_refs(z, k, 3))
    return _REFS[name]


def _walk(name, got_plan, got_cycle, got_states, K_field, K_scalar, gated=None):
    """-> [(stage, deviation, bound)]; raises vfill_trace.StageError at the first stage outside its bound."""
    z, k, v, plan, (c64, c32), (s64, s32) = _refs(name)
    T.compare_plan([lv["fix"] for lv in got_plan.lv], plan)
    out = T.compare_cycle("mg/cycle1", got_cycle, c64, c32, K=K_field)
    return out + T.compare_states("pcg", got_states, s64, s32, lambda p: T.neg_lap(p, k), K_field=K_field, K_scalar=K_scalar,
                                  gated=gated)


def _mirror32(name, mut=None):
    z, k, v = _refs(name)[:3]
    with mutant(mut, z, k):
        plan = M.Plan(k, np.float32, fma=True)
        tr = {}
        M.vcycle(plan, v, trace=tr)
        st = {"stop": 4}
        M.solve_pcg(z, k, tol=0.0, max_cycles=4, dt=np.float32, trace=st, fma=True)
    return plan, tr, st["states"]


def _first_failure(name, mut):
    """-> (the first stage at which the mutant leaves the GPU test's bound, its deviation in units of that bound: inf at a stage
    that is compared exactly), or None when every stage passes."""
    got = _mirror32(name, mut)
    try:
        _walk(name, *got, T.K_FIELD, T.K_SCALAR)
    except T.StageError as e:
        return e.stage, e.over
    return None


@pytest.mark.parametrize("name", T.CASES)
def test_unmutated_mirror_passes_every_stage_with_K_1(name):
    got = _mirror32(name)
    gated = []
    res = _walk(name, *got, 1.0, 1.0, gated)
    L = got[0].L
    # nothing is skipped: every level's down, f and up of the cycle; per pcg state the ten stages compared with the mirrors,
    # less the scalars that have no reference, which are exactly the expected ones
    assert set(gated) == set(T.PCG_GATED[name]) and len(gated) == len(T.PCG_GATED[name]), sorted(gated)
    assert len(res) == (2 * (L - 1) + L) + 4 * 10 - len(gated)
    if L == 1:
        assert [s for s, _, _ in res[:1]] == ["mg/cycle1/L0/up"]      # a one-level raster has no f and no down pass
    z, k = T.case(name)
    for inner in (1, 3):
        b64, b32 = T.bih_refs(z, k, 2, inner)
        g = []
        n = len(T.compare_states(f"bih{inner}", b32, b64, b32, lambda p: B.apply_A(p, k), 1.0, 1.0, gated=g, dot_tol=2.0 ** -30))
        assert n == 3 * 10 - len(g) and all(q.split("/")[1] != "start" for q in g), g


# (mutant, case) -> the stage at which the mutant first leaves the bound; None: every stage must pass, the mutation touches
# nothing on that case or moves it by rounding only.
_MULTI = ("70x135", "33x65", "1x300", "300x1", "3x131500")
_ALL = T.CASES
EXPECTED = {
    # the coarse correction first exists on the highest level with a free cell next to a free coarser cell; one level has no
    # transfer and the checkerboard no free coarse cell
    "prolongation piecewise constant": {"70x135": "mg/cycle1/L3/up", "33x65": "mg/cycle1/L2/up", "1x300": "mg/cycle1/L3/up",
                                        "300x1": "mg/cycle1/L3/up", "3x131500": "mg/cycle1/L2/up"},
    "restriction drops a child": {n: "mg/cycle1/L1/f" for n in _MULTI},
    "no x2 on a level one cell high or wide": {"1x300": "mg/cycle1/L1/f", "300x1": "mg/cycle1/L1/f",
                                               "3x131500": "mg/cycle1/L3/f"},    # heights 3, 2, 1: level 2 is the first
    # the lines' coarsest level has one free cell, which a plain sweep solves as well; the 3-row raster's has none
    "coarsest level: 2 plain sweeps": {"70x135": "mg/cycle1/L4/up", "33x65": "mg/cycle1/L3/up", "5x7": "mg/cycle1/L0/up",
                                       "16x16": "mg/cycle1/L0/up"},
    "correction lost in a band": {n: "mg/cycle1/L0/up" for n in _MULTI},
    # on the checkerboard one sweep solves every unknown (all its neighbours are known) and the second moves a last bit: the
    # fields stay within their bounds and the scalars that this reaches have no reference there
    "one sweep on the up pass": {"70x135": "mg/cycle1/L3/up", "33x65": "mg/cycle1/L2/up", "1x300": "mg/cycle1/L3/up",
                                 "300x1": "mg/cycle1/L3/up", "3x131500": "mg/cycle1/L2/up"},
    "all children fixed": {n: "setup/L1/fix" for n in _MULTI + ("37x53 checkerboard",)},
    # the scalars against the state's own vectors; on 300 x 1 the tile with the most unknowns carries little of r.z
    "pcg: a block dropped from the dots": {**{n: "pcg/start/rz_new.dot" for n in _ALL}, "300x1": "pcg/start/pap.dot"},
    # beta against the state's own scalars: r'.z of the old z is small at iteration 1 but not 0, and the two betas differ in fp32
    "pcg: Fletcher-Reeves beta": {n: "pcg/iter1/beta.formula" for n in _ALL},
    "pcg: p not zeroed at the fixed cells": {n: "pcg/start/pap.dot" for n in _ALL},
}


@pytest.mark.parametrize("name", T.CASES)
@pytest.mark.parametrize("mut", list(MUTANTS))
def test_mutant_fails_at_its_stage_with_margin(mut, name):
    """The first failing stage is the expected one, and the mutant is at least MARGIN x the bound away at that stage."""
    want = EXPECTED[mut].get(name)
    got = _first_failure(name, mut)
    print(mut, "|", name, "|", got)
    if want is None:
        assert got is None, (mut, name, got)
        return
    assert got is not None, f"{mut} on {name}: every stage passed"
    stage, over = got
    assert stage == want, (mut, name, stage, want)
    assert over >= MARGIN, f"{mut} on {name}: {stage} is only {over:.1f} x the bound"


def test_every_mutant_is_caught():
    assert all(EXPECTED[m].get("70x135") or m.startswith("no x2") for m in MUTANTS)
    assert all(any(EXPECTED[m].values()) for m in MUTANTS)


def test_K_follows_from_the_measured_ratios():
    """tests/golden/vfill_stage_ratios.json: the MI355X's deviation from the fp64 mirror and the unit of the bound, per case,
    solver and stage, as measured with K left open.  K is the next power of two above twice the worst ratio."""
    import json
    import math
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vfill_stage_ratios.json")) as fh:
        rows = json.load(fh)["rows"]
    assert {k.rsplit("/", 1)[0] for k in rows} == set(T.CASES)
    assert {k.rsplit("/", 1)[1] for k in rows} == {"mg", "pcg", "bih1", "bih3"}
    worst = {"field": 0.0, "scalar": 0.0}
    for stages in rows.values():
        for stage, (dev, unit) in stages.items():
            kind = "scalar" if stage.rsplit("/", 1)[1].replace("part_", "") in T.SCALARS else "field"
            assert unit > 0 or dev == 0, stage
            worst[kind] = max(worst[kind], dev / unit if unit else 0.0)
    print(worst)
    assert T.K_FIELD == 2.0 ** (math.floor(math.log2(2 * worst["field"])) + 1)
    assert T.K_SCALAR == 2.0 ** (math.floor(math.log2(2 * worst["scalar"])) + 1)


def test_scalar_block_fits_its_slot():
    from mvp_gan.src.fill_voids import ALIGN, VFILL_PCG_SCAL
    assert VFILL_PCG_SCAL.itemsize <= 256 == ALIGN
    assert [VFILL_PCG_SCAL.fields[n][1] for n in VFILL_PCG_SCAL.names] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    assert VFILL_PCG_SCAL.itemsize == 56
    from mvp_gan.src.fill_voids import VFILL_HDR
    assert VFILL_HDR.itemsize == 152 <= ALIGN and VFILL_HDR.fields["c"][1] == 16 and VFILL_HDR.fields["ntiles"][1] == 24


# ---- tracing changes nothing ----------------------------------------------------------------------------------------------
def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["70x135", "5x7", "1x300"])
def test_tracing_leaves_the_results_bit_identical(name):
    z, k = T.case(name)
    for dt in (np.float32, np.float64):
        plan = M.Plan(k, dt)
        v = M._start(z, k, dt)[0]
        assert _eq(M.vcycle(plan, v), M.vcycle(plan, v, trace={}))
        a, ia = M.solve_pcg(z, k, dt=dt)
        tr = {}
        b, ib = M.solve_pcg(z, k, dt=dt, trace=tr)
        assert _eq(a, b) and ia == ib and len(tr["states"]) == ia["cycles"]
        a, ia = B.solve(z, k, dt_in=dt, max_cycles=12)
        tr = {}
        b, ib = B.solve(z, k, dt_in=dt, max_cycles=12, trace=tr)
        assert _eq(a, b) and ia == ib and len(tr["states"]) == ia["cycles"]


# ---- the gap: what the GPU suites assert on the converged result, applied to the mutants ------------------------------------
def test_converged_assertions_pass_the_mutants():
    """The table of DESIGN.md section 8af on the 70 x 135 case: the mutants of the cycle move the level-0 field of the first cycle
    by 1e-2 to 2e-1 of the range, and the assertions on the converged result (max |u - u*| <= 2e-5 x range, cycles <= 50, pcg
    iterations <= mg cycles) still pass.  The table's figures are asserted: the moves to a factor 1.5, the counts to +-1 (a
    count can sit on the stop rule's edge, where the order of a BLAS sum decides)."""
    table = {None: (0.0, 20, 8), "prolongation piecewise constant": (3.1e-2, 34, 9), "restriction drops a child": (1.9e-1, 42, 16),
             "coarsest level: 2 plain sweeps": (1.2e-2, 16, 8), "correction lost in a band": (2.0e-1, 48, 21)}
    name = "70x135"
    z, k, v, plan, (c64, c32), _ = _refs(name)
    rng = float(z[k].max()) - float(z[k].min())
    exact, _ = M.solve_mg(z, k, tol=0.0, max_cycles=60, dt=np.float64)
    rows = []
    for mut in (None, "prolongation piecewise constant", "restriction drops a child", "coarsest level: 2 plain sweeps",
                "correction lost in a band"):
        with mutant(mut, z, k):
            first = M.vcycle(M.Plan(k, np.float32), v)
            a, ia = M.solve_mg(z, k)
            b, ib = M.solve_pcg(z, k)
        base = first if mut is None else base
        moved = float(np.abs(first.astype(np.float64) - base).max()) / rng
        err = max(float(np.abs(x.astype(np.float64) - exact).max()) for x in (a, b)) / rng
        mg_ok = ia["converged"] and ia["cycles"] <= 50 and float(np.abs(a.astype(np.float64) - exact).max()) <= 2e-5 * rng
        pcg_ok = ib["converged"] and ib["cycles"] <= 50 and ib["restarts"] == 0 and \
            float(np.abs(b.astype(np.float64) - exact).max()) <= 2e-5 * rng and \
            ib["cycles"] <= (ia["cycles"] if ia["converged"] else 60)
        rows.append((mut, moved, ia["cycles"], ia["converged"], ib["cycles"], err, mg_ok, pcg_ok))
        print(f"| {mut or 'none'} | {moved:.1e} | {ia['cycles']}{'' if ia['converged'] else ', not converged'} | {ib['cycles']} | "
              f"{err:.1e} | mg {'passes' if mg_ok else 'fails'}, pcg {'passes' if pcg_ok else 'fails'} |")
    assert rows[0][1] == 0.0 and rows[0][6] and rows[0][7]
    for mut, moved, mg_cycles, _conv, pcg_cycles, *_rest in rows:
        want = table[mut]
        assert want[0] / 1.5 <= moved <= want[0] * 1.5 and abs(mg_cycles - want[1]) <= 1 and abs(pcg_cycles - want[2]) <= 1, \
            (mut, moved, mg_cycles, pcg_cycles, want)
    for mut, moved, *_rest, mg_ok, pcg_ok in rows[1:]:
        assert moved >= 1e-2, (mut, moved)                       # six orders above the mirrors' fp32-to-fp64 spread (2e-8)
        assert pcg_ok, mut                                       # the converged pcg result hides every one of them
    assert all(r[6] for r in rows[1:4])                          # and so does the plain solver's; the lost band is left open
