"""CPU checks of what tests/test_hip_wino_routes.py relies on (no GPU, no package import): the Winograd-domain oracle of
tests/conv_oracle.py and the case table of tests/wino_cases.py.

  - the oracle's value = float64 autograd on every case, bit for bit on the integer data;
  - the two regroupings (space-to-depth 5x5 stride 2, shifted space-to-depth 4x4 stride 2) and the Winograd-domain evaluation
    itself = the direct oracle;
  - every exact run meets its exactness conditions, every real run the sensitivity cap (max bound <= 0.05 rms);
  - an fp32 emulation of each algorithm, written here independently of the oracle's evaluation (transforms as 1-D passes,
    per-point contraction, output transform, all in float32): inside the a-priori bound on the real data, the reference's bits on
    the integer data, under a bf16 rounding of the transformed operands too;
  - the rounded run of the bf16 kernels: its data lie on the grid where the fp32 transforms are exact (the emulation's transformed
    operands = the float64 ones, bit for bit), bf16 rounding changes at least 40 % of every transformed operand and 5 % are exact
    ties, the emulation with round-to-nearest-even stays inside the bound, and truncation, round-half-away, a rounding of
    x / w / dy ahead of the transforms and no rounding at all each leave it;
  - `predict`, the Python restatement of the planners, = the table's literal expectations."""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_cases as CC
from tests import conv_oracle as CO
from tests import wino_cases as WC


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double().permute(0, 3, 1, 2)


def autograd64(case, d, mode):
    """The case's op by float64 autograd, in the oracle's layouts."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    x, w = _nchw(d["x"]).requires_grad_(True), _nchw(d["w"]).requires_grad_(True)
    m = None if d["mask"] is None else torch.from_numpy(d["mask"]).double()[:, None]
    if case.op == "fwd":
        z = F.conv2d(x if m is None else x * m, w, None if d["bias"] is None else torch.from_numpy(d["bias"]).double(), s, pad)
        if d["ratio"] is not None:
            z = z * torch.from_numpy(d["ratio"]).double()[:, None]
        a, sl = WC.fwd_act(case, mode)
        y = F.relu(z) if a == CO.ACT_RELU else F.leaky_relu(z, sl) if a == CO.ACT_LEAKY else z
        return {"y": y.detach().permute(0, 2, 3, 1).numpy()}
    dy = _nchw(d["dy"])
    z = F.conv2d(x, w, None, s, pad)
    if case.op == "dgrad":
        dx = torch.autograd.grad(z, x, dy)[0].permute(0, 2, 3, 1).numpy()
        if m is not None:
            dx = dx * d["mask"].astype(np.float64)[..., None]
        if d["gate"] is not None:
            ga, gs = WC.gate_act(case, mode)
            dx = dx * np.where(d["gate"].astype(np.float64) > 0, 1.0, gs if ga == CO.ACT_LEAKY else 0.0)
        if d["base"] is not None:
            dx = dx + d["base"].astype(np.float64)
        return {"dx": dx}
    out = {"dw": torch.autograd.grad(z, w, dy)[0].permute(0, 2, 3, 1).numpy()}
    if "bias" in case.mods:
        out["db"] = d["dy"].astype(np.float64).sum(axis=(0, 1, 2))
    return out


# ---- an fp32 emulation of the algorithms, independent of conv_oracle.wino_corr / wino_wcorr ------------------------------------------
F32 = np.float32


def bf16_round(a):
    """fp32 -> nearest bf16 (ties to even) -> fp32."""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(F32)


def _pass(M, rows):
    """out[i] = sum_j M[i][j] rows[j], one multiply-add at a time in float32 (M's zeros skipped)."""
    out = []
    for i in range(M.shape[0]):
        acc = None
        for j in range(M.shape[1]):
            if M[i, j] != 0:
                t = F32(M[i, j]) * rows[j]
                acc = t if acc is None else acc + t
        out.append(acc)
    return out


def _transform(M, t):
    """M t Mt over a grid t[i][j] of float32 arrays: rows, then columns."""
    n = len(t)
    cols = [_pass(M, [t[i][j] for i in range(n)]) for j in range(len(t[0]))]           # cols[j][a]
    return [_pass(M, [cols[j][a] for j in range(len(cols))]) for a in range(M.shape[0])]        # [a][b]


def _grid_of_tiles(xp, step, size, ty, tx):
    """t[i][j] = the (i, j) element of every tile, [B][ty][tx][C]; zeros beyond the array."""
    B, Hp, Wp, C = xp.shape
    big = np.zeros((B, (ty - 1) * step + size + step, (tx - 1) * step + size + step, C), F32)
    hh, ww = min(Hp, big.shape[1]), min(Wp, big.shape[2])
    big[:, :hh, :ww] = xp[:, :hh, :ww]
    return [[big[:, i::step, j::step][:, :ty, :tx] for j in range(size)] for i in range(size)]


def bf16_half_away(a):
    """fp32 -> bf16 with ties away from zero -> fp32: a WRONG conversion (the kernels round ties to even)."""
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((u + np.uint32(0x8000)) & np.uint32(0xFFFF0000)).view(F32)


def make_emulation(rnd=None, seen=None):
    """(corr, wcorr) for conv_oracle's reducers.  `rnd`: what the transformed operands pass through before the products (None:
    nothing).  `seen`: a list that receives the transformed operands BEFORE `rnd`, as the float32 grids the transforms left."""
    rnd = rnd or (lambda a: a)

    def corr(xp, w, alg, OH, OW):
        Bt, G, At = CO.WINO[alg]
        m, a = At.shape[0], Bt.shape[0]
        ty, tx = -(-OH // m), -(-OW // m)
        V = _transform(Bt, _grid_of_tiles(np.asarray(xp, F32), m, a, ty, tx))
        wf = np.asarray(w, F32)
        U = _transform(G, [[wf[:, u, v, :] for v in range(G.shape[1])] for u in range(G.shape[1])])        # [a][a] of [N][C]
        if seen is not None:
            seen.append((V, U))
        Mm = [[np.matmul(rnd(V[i][j]), rnd(U[i][j]).T) for j in range(a)] for i in range(a)]
        Y = _transform(At, Mm)
        B, N = xp.shape[0], w.shape[0]
        y = np.zeros((B, ty * m, tx * m, N), F32)
        for i in range(m):
            for j in range(m):
                y[:, i::m, j::m] = Y[i][j]
        return y[:, :OH, :OW], 0.0, 0.0

    def wcorr(xp, dy, alg):
        Bt, G, At = CO.WINO[alg]
        m, a = At.shape[0], Bt.shape[0]
        B, OH, OW, N = dy.shape
        ty, tx = -(-OH // m), -(-OW // m)
        V = _transform(Bt, _grid_of_tiles(np.asarray(xp, F32), m, a, ty, tx))
        Yt = _transform(np.ascontiguousarray(At.T), _grid_of_tiles(np.asarray(dy, F32), m, m, ty, tx))
        if seen is not None:
            seen.append((V, Yt))
        C = xp.shape[3]
        Mm = [[np.matmul(rnd(Yt[i][j]).reshape(-1, N).T, rnd(V[i][j]).reshape(-1, C)) for j in range(a)] for i in range(a)]
        D = _transform(np.ascontiguousarray(G.T), Mm)                                # [u][v] of [N][C]
        dw = np.stack([np.stack(r, axis=1) for r in D], axis=1)                      # [N][u][v][C]
        return dw, 0.0, 0.0, B * ty * tx

    return corr, wcorr


def emulate(case, d, mode, bf16=False, rnd=None, pre=None, seen=None):
    """The case's op as the kernels compute it: operands and epilogue in float32, the algorithm of the case's route.  `bf16`: the
    transformed operands through bf16_round (`rnd`: through that instead).  `pre`: the two MFMA operands of the op pass through it
    AHEAD of the transforms -- a wrong place to round."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    corr, wcorr = make_emulation(rnd or (bf16_round if bf16 else None), seen)
    if pre is not None:
        d = dict(d, **{name: pre(d[name]) for name in CC.OPERANDS[case.op]})
    one = F32(1.0)
    if case.op == "fwd":
        xin = d["x"] if d["mask"] is None else d["x"] * d["mask"][..., None]
        (z, _, _), _ = CO._wino_fwd_corr(xin.astype(F32), d["w"], k, s, pad, case.alg, False, corr)
        if d["bias"] is not None:
            z = z + d["bias"]
        if d["ratio"] is not None:
            z = z * d["ratio"][..., None]
        a, sl = WC.fwd_act(case, mode)
        y = np.where(z > 0, z, z * F32(sl if a == CO.ACT_LEAKY else 0.0)) if a != CO.ACT_NONE else z
        return {"y": y.astype(F32)}
    if case.op == "dgrad":
        dx, _, _ = CO._wino_dgrad_corr(d["dy"], d["w"], (B, H, W, Cin), k, s, pad, case.alg, False, corr)
        if d["mask"] is not None:
            dx = dx * d["mask"][..., None]
        if d["gate"] is not None:
            ga, gs = WC.gate_act(case, mode)
            dx = dx * np.where(d["gate"] > 0, one, F32(gs if ga == CO.ACT_LEAKY else 0.0))
        if d["base"] is not None:
            dx = dx + d["base"]
        return {"dx": dx.astype(F32)}
    dw = CO._wino_wgrad_corr(d["x"], d["dy"], k, s, pad, case.alg, False, wcorr)[0]
    return {"dw": np.asarray(dw, F32)}


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------
def test_transform_pass_roundings_come_from_the_matrices():
    assert [CO.wino_T(a) for a in ("F23", "F22", "F43")] == [26, 18, 42]
    assert (CO.wino_T("F23", wgrad=True), CO.wino_T("F22", wgrad=True)) == (22, 18)


@pytest.mark.parametrize("geom,alg", [((2, 17, 19, 8, 4, 3, 1, 1), "F23"), ((1, 17, 19, 8, 4, 3, 1, 0), "F23"),
                                      ((1, 15, 17, 8, 4, 3, 1, 2), "F23"), ((1, 19, 37, 8, 4, 3, 1, 1), "F43"),
                                      ((2, 12, 16, 4, 3, 5, 2, 2), "F23"), ((2, 14, 18, 4, 3, 4, 2, 1), "F22")])
def test_winograd_domain_and_regroupings_equal_the_direct_oracle(geom, alg):
    B, H, W, Cin, Cout, k, s, p = geom
    rng = np.random.default_rng(sum(geom))
    x, w = rng.integers(-3, 4, (B, H, W, Cin)).astype(float), rng.integers(-3, 4, (Cout, k, k, Cin)).astype(float)
    dy = rng.integers(-3, 4, (B, CO.out_size(H, k, s, p), CO.out_size(W, k, s, p), Cout)).astype(float)
    tol = 0.0 if alg != "F43" else 1e-11            # (1/6 and 1/24 are not float64 numbers)
    (y, _, _), K = CO._wino_fwd_corr(x, w, k, s, p, alg, False)
    assert K == (Cin if k == 3 else 4 * Cin)
    assert np.abs(y - CO.conv_fwd(x, w, k, s, p).val).max() <= tol
    dx = CO._wino_dgrad_corr(dy, w, (B, H, W, Cin), k, s, p, alg, False)[0]
    assert np.abs(dx - CO.conv_dgrad(dy, w, (B, H, W, Cin), k, s, p).val).max() <= tol
    if alg != "F43":
        dw, _, _, ntiles = CO._wino_wgrad_corr(x, dy, k, s, p, alg, False)
        assert ntiles == B * -(-dy.shape[1] // 2) * -(-dy.shape[2] // 2)
        assert np.array_equal(dw, CO.conv_wgrad(x, dy, k, s, p)[0].val)
    # S_w is never below the direct sum of absolute values (|sum of products| <= the sum of their magnitudes, term by term)
    Sd = CO.conv_fwd(np.abs(x), np.abs(w), k, s, p).val
    assert (CO.wino_fwd(x, w, k, s, p, alg).S >= Sd - 1e-9).all()


def test_predict_equals_the_table():
    bad = []
    for c in WC.CASES:
        rec, sp = WC.predict(c)
        if rec != c.expect or not WC.splits_ok(c.splits, sp):
            bad.append((c.id, rec, sp, c.expect, c.splits))
    assert not bad, bad


def test_the_table_reaches_every_variant():
    seen = {r for c in WC.CASES for r in c.expect}
    want = {(0, 4064, r) for r in range(1, 17)} | {(3, 4016, r) for r in range(1, 9)} | {(0, 4022, r) for r in range(1, 9)} | \
           {(0, 4044, r) for r in (1, 2, 3)} | {WC.WG, WC.WG16, WC.WG22}
    assert want <= seen, sorted(want - seen)


@pytest.mark.parametrize("case", WC.CASES, ids=[c.id for c in WC.CASES])
def test_oracle_conditions_and_emulation(case):
    t0 = time.perf_counter()
    bf16 = case.prec == "bf16"
    for mode in (m for m in case.runs if m != "rounded"):           # the rounded run: test_rounded_run_tells_the_conversions_apart
        d = WC.make_inputs(case, mode)
        ref = WC.reference(case, d, mode)
        gold = autograd64(case, d, mode)
        emu = emulate(case, d, mode, bf16 and mode == "exact")
        slabs = WC.slab_cap(case, case.expect)
        for name, r in ref.items():
            if mode == "exact":
                assert np.array_equal(r.val, gold[name]), (case.id, name)
                if name == "db":
                    assert CO.exact_ok(r)
                    continue
                assert CO.wino_exact_ok(r, bf16), (case.id, name, float(r.S.max()), r.vmax, r.umax)
                assert np.array_equal(emu[name].astype(np.float64), r.val), \
                    f"{case.id} {name}: the fp32{' / bf16' if bf16 else ''} emulation misses the integer reference"
                if not bf16:        # the bf16 rounding is the identity where the condition holds: ask it of every exact case that meets it
                    if CO.wino_exact_ok(r, True):
                        assert np.array_equal(emulate(case, d, mode, True)[name].astype(np.float64), r.val), (case.id, name)
            else:
                assert np.allclose(r.val, gold[name], rtol=1e-11, atol=1e-11), (case.id, name)
                if name in emu:
                    q, where = CO.worst(emu[name], r, slabs)
                    print(f"EMULATION_ERR_OVER_BOUND {case.id} {name} {q:.4f}")
                    assert q <= 1.0, (case.id, name, q, where)
        if mode == "real":
            sens = WC.sensitivity(case, ref)
            print(f"SENSITIVITY {case.id} {sens:.2e}")
            assert sens <= WC.SENSITIVITY_CAP, (case.id, sens)
    print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")


# ---- the rounded run of the bf16 Winograd kernels: conditions on inputs and reference, checked without the kernels ----------------------
ROUNDED = [c for c in WC.CASES if "rounded" in c.runs]
CHANGED_MIN, TIES_MIN = 0.40, 0.05


def _operands64(case, d):
    """The float64 transformed operands of the case, [(first, second), ...] per stride-1 problem, through the oracle's reducers."""
    B, H, W, Cin, Cout, k, s, pad = case.geom
    seen = []

    def corr(xp, w, alg, OH, OW):
        seen.append(CO.wino_operands(xp, w, alg, OH, OW))
        return CO.wino_corr(xp, w, alg, OH, OW)

    def wcorr(xp, dy, alg):
        seen.append(CO.wino_woperands(xp, dy, alg))
        return CO.wino_wcorr(xp, dy, alg)

    if case.op == "fwd":
        xin = CO.f64(d["x"]) if d["mask"] is None else CO.f64(d["x"]) * CO.f64(d["mask"])[..., None]
        CO._wino_fwd_corr(xin, CO.f64(d["w"]), k, s, pad, case.alg, False, corr)
    elif case.op == "dgrad":
        CO._wino_dgrad_corr(CO.f64(d["dy"]), CO.f64(d["w"]), (B, H, W, Cin), k, s, pad, case.alg, False, corr)
    else:
        CO._wino_wgrad_corr(CO.f64(d["x"]), CO.f64(d["dy"]), k, s, pad, case.alg, False, wcorr)
    return seen


def _as_array(t, like):
    """An emulation operand (a grid [i][j] of float32 arrays) in the layout of the oracle's `like`."""
    g = np.stack([np.stack(row) for row in t])                      # [a][a] + the array's own axes
    return g if g.shape == like.shape else np.moveaxis(g, (0, 1), (-2, -1))


def test_the_rounded_run_covers_the_bf16_winograd_cases():
    want = {c.id for c in WC.CASES if c.prec == "bf16" and c.expect[0][:2] in ((3, 4016), (3, 4116))}
    assert {c.id for c in ROUNDED} == want and len(want) >= 21
    assert WC.BY_ID["w16_keeps_fp32_wgrad"].runs == ("exact",)
    assert {c.env for c in ROUNDED} == {None, "TG_WINO_NO_PIPE", "TG_WINO_NO_FAST"}
    assert {r for c in ROUNDED for r in c.expect} == {(3, 4016, r) for r in range(1, 9)} | {WC.WG16}


def test_half_away_and_truncation_differ_from_rne_where_they_should():
    a = np.array([1.0, 257.0, 258.0, 259.0, 261.0, -257.0, -259.0, 1029.0], F32)      # 257, 259, 261: ties of the step-2 binade
    assert CO.bf16_rne(a).tolist() == bf16_round(a).tolist() == [1.0, 256.0, 258.0, 260.0, 260.0, -256.0, -260.0, 1032.0]
    assert bf16_half_away(a).tolist() == [1.0, 258.0, 258.0, 260.0, 262.0, -258.0, -260.0, 1032.0]
    assert CO.bf16_trunc(a).tolist() == [1.0, 256.0, 258.0, 258.0, 260.0, -256.0, -258.0, 1024.0]


@pytest.mark.parametrize("case", ROUNDED, ids=[c.id for c in ROUNDED])
def test_rounded_run_tells_the_conversions_apart(case):
    t0 = time.perf_counter()
    d = WC.make_inputs(case, "rounded")
    ref = WC.reference(case, d, "rounded")               # asserts wino_grid_ok where it rounds
    slabs = WC.slab_cap(case, case.expect)
    # the grid: every transformed operand is an integer number of quanta below 2^24, and the fp32 transforms reproduce it bit for bit
    Bt, G, At = CO.WINO[case.alg]
    mats = (Bt, At.T) if case.op == "wgrad" else (Bt, G)
    raw = [d[n] for n in CC.OPERANDS[case.op]]             # (x, w) | (dy, w) | (x, dy): the order of the transformed pairs
    seen = []
    emu = emulate(case, d, "rounded", True, seen=seen)
    ops64 = _operands64(case, d)
    assert len(seen) == len(ops64) == 1
    for which, (t64, t32) in enumerate(zip(ops64[0], seen[0])):
        t32 = _as_array(t32, t64)
        assert t32.dtype == F32 and np.array_equal(t32.astype(np.float64), t64), (case.id, which)
        bits = np.ascontiguousarray(t32).view(np.uint32)
        changed = float(np.mean(CO.bf16_rne(t32) != t32))
        ties = float(np.mean((bits & np.uint32(0xFFFF)) == np.uint32(0x8000)))
        print(f"ROUNDING_MATTERS {case.id} operand{which} changed={changed:.3f} ties={ties:.3f}")
        assert changed >= CHANGED_MIN and ties >= TIES_MIN, (case.id, which, changed, ties)
    assert CO.wino_grid_ok(case.alg, mats, raw, ops64[0])
    # the reference itself: rounding moves it (the unrounded oracle is another function), db stays the plain column sum
    plain = WC.reference(case, d, "real")
    for name, r in ref.items():
        if name == "db":
            assert np.array_equal(r.val, d["dy"].astype(np.float64).sum(axis=(0, 1, 2)))
        else:
            q, _ = CO.worst(plain[name].val, r, slabs)
            print(f"EMULATION_ERR_OVER_BOUND {case.id} {name} unrounded_convolution {q:.1f}")
            assert q > 1.0, (case.id, name, q)
    sens = WC.sensitivity(case, ref)
    print(f"SENSITIVITY {case.id} {sens:.2e}")
    assert sens <= WC.SENSITIVITY_CAP, (case.id, sens)
    # round-to-nearest-even at the transformed operands is inside the bound; every other conversion is outside
    wrong = {"trunc": dict(rnd=CO.bf16_trunc), "half_away": dict(rnd=bf16_half_away), "rounded_before": dict(pre=bf16_round)}
    for name in emu:
        q, where = CO.worst(emu[name], ref[name], slabs)
        print(f"EMULATION_ERR_OVER_BOUND {case.id} {name} rne {q:.4f}")
        assert q <= 1.0, (case.id, name, q, where)
    for variant, kw in wrong.items():
        out = emulate(case, d, "rounded", **kw)
        for name in out:
            q, _ = CO.worst(out[name], ref[name], slabs)
            over = float(np.mean(np.abs(out[name] - ref[name].val) > CO.bound(ref[name], slabs)))
            print(f"EMULATION_ERR_OVER_BOUND {case.id} {name} {variant} {q:.1f} (elements over the bound: {over:.2f})")
            assert q > 1.0, f"{case.id} {name}: the rounded run cannot tell {variant} from round-to-nearest-even ({q:.3f})"
    print(f"CASE_SECONDS {case.id} {time.perf_counter() - t0:.2f}")
