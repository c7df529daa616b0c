"""CPU checks behind tests/test_hip_batchnorm.py: the numpy oracle tests/bn_oracle.py against float64 autograd, the dispatch mirror
of tests/bn_cases.py against the library's host-side queries, the coverage the case tables claim, and the conditions under which
the GPU file may ask for bit-equality (every fp32 sum exact in any order) or apply its derived bounds.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bn_cases as BC
from tests import bn_oracle as BO


def _rel(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / max(float(np.abs(ref).max()), 1e-300))


# ---- the oracle against float64 autograd ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C,act,with_ratio", [(37, 5, BO.ACT_RELU, True), (256, 16, BO.ACT_LEAKY, False), (101, 64, BO.ACT_NONE, True)])
def test_oracle_equals_float64_autograd(rows, C, act, with_ratio):
    """The model behind ratio and dbias: the conv output that feeds BatchNorm is y = ratio * (x W + bias) per row (partial conv), so
    autograd's gradient of x W is ratio * d loss / d y (the kernels' dy) and that of the bias its sum over the rows (dbias)."""
    g = torch.Generator().manual_seed(rows + C)
    xw = (torch.randn(rows, C, generator=g, dtype=torch.float64) * 1.5 + 0.7).requires_grad_(True)
    bias = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64, requires_grad=True)
    ratio = torch.rand(rows, generator=g, dtype=torch.float64) + 0.5 if with_ratio else None
    dout = torch.randn(rows, C, generator=g, dtype=torch.float64)
    eps, mom, slope = 1e-5, 0.1, 0.2
    rm, rv = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    y = (xw + bias) if ratio is None else (xw + bias) * ratio[:, None]
    z = F.batch_norm(y, rm, rv, gamma, beta, True, mom, eps)
    out = z if act == BO.ACT_NONE else (F.relu(z) if act == BO.ACT_RELU else F.leaky_relu(z, slope))
    out.backward(dout)
    yn, gn, bn = y.detach().numpy(), gamma.detach().numpy(), beta.detach().numpy()
    mean, var, rstd = BO.stats(yn, eps)
    assert _rel(BO.apply(yn, mean, rstd, gn, bn, act, slope), out.detach().numpy()) < 1e-12
    nrm, nrv = BO.running(rm0.numpy(), rv0.numpy(), mean, var, rows, mom)
    assert _rel(nrm, rm.numpy()) < 1e-12 and _rel(nrv, rv.numpy()) < 1e-12
    dy, dgamma, dbeta, dbias, q = BO.bwd(dout.numpy(), yn, mean, rstd, gn, bn, act, slope, None if ratio is None else ratio.numpy())
    assert _rel(dy, xw.grad.numpy()) < 1e-12
    assert _rel(dgamma, gamma.grad.numpy()) < 1e-12 and _rel(dbeta, beta.grad.numpy()) < 1e-12
    # dbias (closed form of the five sums) = sum over rows of dy, up to that sum's own rounding: relative to sum |dy|
    scale = float(np.abs(dy).sum(0).max())
    assert float(np.abs(dbias - bias.grad.numpy()).max()) < 1e-12 * scale
    assert float(np.abs(dbias - dy.sum(0)).max()) < 1e-12 * scale
    assert np.array_equal(q[0], dbeta) and np.array_equal(q[1], dgamma)


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 1, 6, 4), (3, 4, 1, 8)])
def test_conv1_dgrad_equals_conv_transpose(shape):
    B, H, W, C = shape
    g = torch.Generator().manual_seed(sum(shape))
    dz = torch.randn(B, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, C, generator=g, dtype=torch.float64)
    # forward conv C -> 1: weight [1][C][3][3]; its input gradient is conv_transpose2d with the same weight
    ref = F.conv_transpose2d(dz[:, None], w.permute(2, 0, 1)[None].contiguous(), None, 1, 1).permute(0, 2, 3, 1)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.permute(2, 0, 1)[None].contiguous(), None, 1, 1).backward(dz[:, None])
    got = BO.conv1_dgrad(dz.numpy(), w.numpy())
    assert _rel(got, ref.numpy()) < 1e-12
    assert _rel(got, x.grad.permute(0, 2, 3, 1).numpy()) < 1e-12


def test_grouped_oracle_is_the_loop_over_passes():
    rng = np.random.default_rng(3)
    rows_g, C, groups = 9, 4, 3
    y, dout = rng.standard_normal((groups * rows_g, C)), rng.standard_normal((groups * rows_g, C))
    gamma, beta = rng.random(C) + 0.5, rng.standard_normal(C)
    mean, var, rstd = BO.stats_grouped(y, groups, 1e-5)
    out = BO.apply_grouped(y, groups, mean, rstd, gamma, beta, BO.ACT_RELU)
    dy, dgamma, dbeta, dbias, per = BO.bwd_grouped(dout, y, groups, mean, rstd, gamma, beta, BO.ACT_RELU)
    for g in range(groups):
        s = slice(g * rows_g, (g + 1) * rows_g)
        m1, v1, r1 = BO.stats(y[s], 1e-5)
        assert np.array_equal(m1, mean[g]) and np.array_equal(r1, rstd[g]) and np.array_equal(v1, var[g])
        assert np.array_equal(out[s], BO.apply(y[s], m1, r1, gamma, beta, BO.ACT_RELU))
        assert np.array_equal(dy[s], BO.bwd(dout[s], y[s], m1, r1, gamma, beta, BO.ACT_RELU)[0])
    assert dgamma.dtype == np.float32 and _rel(dgamma, sum(p[1] for p in per)) < 1e-6
    rm, rv = BO.running_multi(np.zeros(C), np.ones(C), mean, var, rows_g, 0.1, [2, 0, 0])
    a, b = np.zeros(C, np.float32), np.ones(C, np.float32)
    for g in (2, 0, 0):
        a, b = (x.astype(np.float32) for x in BO.running(a, b, mean[g], var[g], rows_g, 0.1))
    assert np.array_equal(rm, a) and np.array_equal(rv, b)


# ---- the mirror against the library ------------------------------------------------------------------------------------------
def test_mirror_agrees_with_the_host_side_queries():
    from tg_hip import lib as L
    lib = L.load()
    rows_list = sorted({1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 683, 1000, 2047, 2048, 2049, 3000, 4095, 4096,
                        4097, 4100, 8191, 8192, 8200, 16383, 16384, 16385, 16500, 16512, 65536, 100000, 262144, 1 << 20, (1 << 20) + 7,
                        16 * 512 * 512} | {r for r, _ in BC.FWD_BWD_CASES} | {b * h * w for b, h, w, _ in BC.CONV1_CASES})
    c_list = sorted(set(range(1, 41)) | {48, 60, 63, 64, 65, 72, 80, 96, 100, 128, 192, 255, 256, 257, 258, 260, 320, 511, 512, 513,
                                         768, 1020, 1023, 1024} | {c for _, c in BC.FWD_BWD_CASES})
    n = 0
    for rows in rows_list:
        for c in c_list:
            n += 1
            assert lib.tg_bn_ws_bytes(rows, c) == BC.bn_ws_bytes(rows, c), (rows, c)
            assert lib.tg_bn_conv1_ws_bytes(rows, c) == BC.bn_conv1_ws_bytes(rows, c), (rows, c)
            assert bool(lib.tg_bn_bwd_conv1_supported(rows, c)) == BC.conv1_supported(rows, c), (rows, c)
            for groups in (1, 2, 3, 8):
                assert lib.tg_bn_grouped_ws_bytes(rows, groups, c) == BC.bn_grouped_ws_bytes(rows, groups, c), (rows, groups, c)
    assert n > 2000
    assert lib.tg_bn_ws_bytes(0, 4) == 0 and lib.tg_bn_grouped_ws_bytes(8, 2, 6) == 0
    for B, H, W, C in BC.CONV1_CASES:
        assert BC.conv1_supported(B * H * W, C), (B, H, W, C)
    assert not BC.conv1_supported(1 * 16 * 64, 128) and not BC.conv1_supported(100, 6)


# ---- what the tables claim to cover -----------------------------------------------------------------------------------------
def _bucket(grid):
    return 0 if grid == 1 else (1 if grid < 16 else (2 if grid < 64 else 3))


def test_tables_reach_every_path_and_geometry():
    tables = {"scalar": BC.SCALAR, "quad": BC.QUAD, "small": BC.SMALL}
    for name, table in tables.items():
        for rows, C in table:
            assert BC.path(rows, C, "bn_fwd") == name and BC.path(rows, C, "bn_act_bwd") == name, (name, rows, C)
            # tg_bn_stats / tg_bn_act_fwd and the grouped calls never take the one-launch form
            assert BC.path(rows, C, "bn_stats") == ("quad" if C % 4 == 0 else "scalar")
        # each path x each activation; ratio, dbias, in-place and running statistics given and absent on each path
        got = [BC.case_opts(BC.FWD_BWD_CASES, c) for c in table]
        assert {o["act"] for o in got} == set(BC.ACTS), name
        for key in ("ratio", "dbias", "inplace", "running"):
            assert {o[key] for o in got} == {True, False}, (name, key)
        assert any(r & (r - 1) == 0 for r, _ in table), name                      # a power-of-two row count
    for rows, C in BC.MIXED:
        assert BC.path(rows, C, "bn_stats") == BC.path(rows, C, "bn_act_fwd") == "quad" and BC.path(rows, C, "bn_fwd") == "small"
    rows, C = BC.APPLY_CAP[0]
    assert BC.path(rows, C, "bn_act_bwd") == "quad" and BC.row_geom(rows, C)["capped"]
    assert not any(BC.row_geom(r, c)["capped"] for r, c in BC.QUAD + BC.SMALL)
    # reduction geometry off the small path (tg_bn_stats reaches it at the SMALL shapes too)
    sc = [BC.first_stage(r, c) for r, c in BC.SCALAR]
    qd = [BC.first_stage(r, c) for r, c in BC.QUAD]                                # what tg_bn_act_bwd reaches; tg_bn_stats adds SMALL + MIXED
    assert {g["npass"] for g in sc} == {1, 2, 4}
    assert any(g["idle"] for g in sc) and any(not g["idle"] for g in sc)
    assert any(g["idle"] for g in qd) and any(not g["idle"] for g in qd)
    assert [g["capped"] for g in sc].count(True) == 1 and BC.col_geom(16500, 257)["grid"] <= 1024
    assert BC.col_geom(16500, 257)["rows_per_block"] * (BC.col_geom(16500, 257)["grid"] - 1) + 1 <= 16500 < \
        BC.col_geom(16500, 257)["rows_per_block"] * BC.col_geom(16500, 257)["grid"]                     # ragged last block
    assert [g["capped"] for g in qd].count(True) == 1 and BC.col_geom4(4100, 1024)["grid"] <= 512
    assert 4100 % BC.col_geom4(4100, 1024)["rows_per_block"] != 0
    for geoms in (sc, qd):
        assert {_bucket(g["grid"]) for g in geoms} == {0, 1, 2, 3}               # final_reduce: 1, < 16, < 64 (rolled), >= 64 (unrolled trip)
    assert any(BC.col_geom4(r, c)["qpp"] == 64 for r, c in BC.QUAD + BC.SMALL + BC.APPLY_CAP) or \
        any(BC.conv1_geom(b * h * w, c)["qpp"] == 64 for b, h, w, c in BC.CONV1_CASES)
    assert any(r == 2 for r, _ in BC.SCALAR) and any(r == 2 for r, _ in BC.QUAD) and any(r == 2 for r, _ in BC.SMALL)
    # conv1: share at every lane-group width, non-share below and above them, H = 1 and W = 1, the first-stage cap
    for case in BC.CONV1_NON_SHARE + BC.CONV1_CAP:
        assert not BC.conv1_geom(case[0] * case[1] * case[2], case[3])["share"], case
    assert [BC.conv1_geom(b * h * w, c)["qpp"] for b, h, w, c in BC.CONV1_SHARE] == [16, 32, 64]
    assert all(BC.conv1_geom(b * h * w, c)["share"] for b, h, w, c in BC.CONV1_SHARE)
    assert {c for _, _, _, c in BC.CONV1_NON_SHARE} >= {512, 1024}
    assert any(h == 1 for _, h, _, _ in BC.CONV1_CASES) and any(w == 1 for _, _, w, _ in BC.CONV1_CASES)
    b, h, w, c = BC.CONV1_CAP[0]
    assert BC.conv1_geom(b * h * w, c)["capped"] and BC.conv1_geom(b * h * w, c)["grid"] <= 2048
    assert not any(BC.conv1_geom(b * h * w, c)["capped"] for b, h, w, c in BC.CONV1_NON_SHARE + BC.CONV1_SHARE)
    assert not any(BC.conv1_geom(b * h * w, c)["apply_capped"] for b, h, w, c in BC.CONV1_CASES)     # left out: > 65536 * rlanes rows
    got = [BC.case_opts(BC.CONV1_CASES, c) for c in BC.CONV1_CASES]
    assert {o["act"] for o in got} == set(BC.ACTS) and {o["ratio"] for o in got} == {True, False} and {o["dbias"] for o in got} == {True, False}
    # grouped: 1 .. 8 groups, the quad first stage with idle threads, full blocks, and its grid cap
    gg = [BC.col_geom4(r, c) for r, c, _ in BC.GROUPED]
    assert any(g["capped"] for g in gg) and any(g["qpp"] * g["rlanes"] < 256 for g in gg) and {_bucket(g["grid"]) for g in gg} == {0, 1, 2, 3}
    assert max(g for _, _, g in BC.GROUPED) == 8 and {BC.case_opts(BC.GROUPED, c)["act"] for c in BC.GROUPED} == set(BC.ACTS)
    assert sorted(len(o) for o in BC.ORDERS) == [3, 4, 8] and all(max(o) < 4 for o in BC.ORDERS)
    assert all(r * c * g < 20_000_000 for r, c, g in BC.GROUPED) and all(r * c < 20_000_000 for r, c in BC.FWD_BWD_CASES)


# ---- exactness of the part A inputs -----------------------------------------------------------------------------------------
def _check_exact_sums(terms, units, rows, tag, rng):
    for i, (t, unit) in enumerate(zip(terms, units)):
        k = t / unit
        assert np.array_equal(k, np.round(k)), (tag, i, "terms are not multiples of the unit")
        assert rows * float(np.abs(k).max()) < 2 ** 24, (tag, i, rows * float(np.abs(k).max()))
        # any order gives the same bits: a strictly sequential fp32 running sum over a random row order, against float64
        seq = np.cumsum(t.astype(np.float32)[rng.permutation(rows)], axis=0, dtype=np.float32)[-1]
        assert np.array_equal(seq.astype(np.float64), t.sum(0)), (tag, i)


@pytest.mark.parametrize("case", BC.FWD_BWD_CASES, ids=BC.case_id)
def test_exact_inputs_make_every_sum_exact(case):
    rows, C = case
    o = BC.case_opts(BC.FWD_BWD_CASES, case)
    p = BC.exact_inputs(rows, C)
    rng = np.random.default_rng(rows + C)
    _check_exact_sums(BC.stat_terms(p["y"]), BC.STAT_UNITS, rows, (case, "stat"), rng)
    terms = BC.bwd_terms(p["dout"], p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, p["ratio"] if o["ratio"] else None)
    _check_exact_sums(terms, BC.BWD_UNITS, rows, (case, "bwd"), rng)
    z = (p["y"].astype(np.float64) - p["mean"]) * p["rstd"] * p["gamma"] + p["beta"]
    assert rows * C < 2000 or (z == 0).any()                                      # the gate's own edge is in the data
    if rows % 2 == 0:
        d = BC.dyadic_stat_inputs(rows, C)
        _check_exact_sums(BC.stat_terms(d["y"]), (0.5, 0.25), rows, (case, "dyadic stat"), rng)
        mean, var, rstd = BO.stats(d["y"], 0.0)
        assert np.array_equal(mean, d["m"]) and np.array_equal(rstd, 1.0 / d["a"])
        terms = BC.bwd_terms(d["dout"], d["y"], d["m"], 1.0 / d["a"], d["gamma"], d["beta"], o["act"], BC.SLOPE, d["ratio"] if o["ratio"] else None)
        _check_exact_sums(terms, BC.BWD_UNITS, rows, (case, "dyadic bwd"), rng)


@pytest.mark.parametrize("case", BC.CONV1_CASES, ids=BC.case_id)
def test_exact_conv1_inputs_make_every_sum_exact(case):
    B, H, W, C = case
    rows = B * H * W
    o = BC.case_opts(BC.CONV1_CASES, case)
    p = BC.exact_conv1_inputs(B, H, W, C)
    dout = BO.conv1_dgrad(p["dz"], p["w"]).reshape(rows, C)
    assert np.array_equal(dout, np.round(dout)) and np.abs(dout).max() <= 9
    terms = BC.bwd_terms(dout, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, p["ratio"] if o["ratio"] else None)
    _check_exact_sums(terms, BC.BWD_UNITS, rows, case, np.random.default_rng(rows))


@pytest.mark.parametrize("case", BC.GROUPED, ids=BC.case_id)
def test_exact_grouped_inputs_make_every_sum_exact(case):
    rows_g, C, groups = case
    o = BC.case_opts(BC.GROUPED, case)
    rng = np.random.default_rng(rows_g)
    p = BC.exact_grouped_inputs(rows_g, C, groups)
    assert len({tuple(m) for m in p["mean"]}) == groups or C * 101 < groups * 8     # the passes' statistics differ
    for g in range(groups):
        s = slice(g * rows_g, (g + 1) * rows_g)
        _check_exact_sums(BC.stat_terms(p["y"][s]), BC.STAT_UNITS, rows_g, (case, g, "stat"), rng)
        terms = BC.bwd_terms(p["dout"][s], p["y"][s], p["mean"][g], p["rstd"][g], p["gamma"], p["beta"], o["act"], BC.SLOPE, None)
        # the bound takes all passes' rows: the parameter gradients are summed over the passes in fp32
        for i, (t, unit) in enumerate(zip(terms, BC.BWD_UNITS)):
            assert rows_g * groups * float(np.abs(t / unit).max()) < 2 ** 24, (case, g, i)
        _check_exact_sums(terms, BC.BWD_UNITS, rows_g, (case, g, "bwd"), rng)


def test_power_of_two_rows_make_dy_exact_in_fp32():
    """Where rows is a power of two the GPU file asks dy bit for bit: the kernels' fp32 formula, evaluated step by step in numpy
    fp32 (each product and difference rounded on its own, the harshest reading), must land on the float64 value."""
    for table in (BC.SCALAR, BC.QUAD, BC.SMALL):
        for rows, C in table:
            if rows & (rows - 1):
                continue
            o = BC.case_opts(BC.FWD_BWD_CASES, (rows, C))
            p = BC.exact_inputs(rows, C)
            ratio = p["ratio"] if o["ratio"] else None
            dy, dgamma, dbeta, _, _ = BO.bwd(p["dout"], p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio)
            f = np.float32
            xh = (p["y"] - p["mean"]) * p["rstd"]
            z = xh * p["gamma"] + p["beta"]
            ga = np.ones_like(z) if o["act"] == BO.ACT_NONE else np.where(z > 0, f(1), f(0) if o["act"] == BO.ACT_RELU else f(BC.SLOPE))
            g = p["dout"] * ga
            inv_n = f(1.0) / f(rows)
            v = p["gamma"] * p["rstd"] * (g - dbeta.astype(f) * inv_n - xh * dgamma.astype(f) * inv_n)
            if ratio is not None:
                v = v * ratio[:, None]
            assert v.dtype == np.float32 and np.array_equal(v.astype(np.float64), dy), (rows, C)


# ---- the condition of the part B bounds ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BC.REAL_CASES, ids=BC.case_id)
def test_real_inputs_keep_the_variance_bound_small(case):
    _, rows, C, groups = case
    for kind in BC.REAL_KINDS:
        p = BC.real_inputs(kind, rows, C, groups)
        assert p["y"].shape == (groups * rows, C) and np.isfinite(p["y"]).all()
        for g in range(groups):
            b = BC.stat_bounds(p["y"][g * rows:(g + 1) * rows], BC.EPS32)
            frac = b["b_var"] / (b["var"] + BC.EPS32)
            assert float(frac.max()) <= 0.05, (case, kind, float(frac.max()))
            if kind == "const":
                assert b["var"][p["const_channel"]] == 0.0 and b["b_var"][p["const_channel"]] == 0.0
            if kind == "outlier" and rows > 2:
                y = p["y"][g * rows:(g + 1) * rows].astype(np.float64)
                assert float(((y[0] - y[1:].mean(0)) / 0.01).min()) > 6.0                 # in units of the distribution's std
