"""The BatchNorm family of csrc/pointwise.hip -- the shifted-sum statistics, the one-launch small-map kernels, the grouped (stacked
passes) kernels, the backward over a recomputed 1-channel dgrad, the running-statistics updates -- through tg_hip.ops against the
numpy fp64 oracle tests/bn_oracle.py, on the shapes of tests/bn_cases.py (one per reduction geometry; which kernel a shape
reaches is known from the mirror there, checked on the CPU by tests/test_bn_oracle_cpu.py).

Part A, exact.  The inputs are small dyadic numbers, so every fp32 sum the kernels form -- per thread, per block, over blocks -- is
exact in any order and the kernel must give the oracle's bits: dgamma, dbeta, dy where rows is a power of two (else dy within
8 * 2^-24 of the formula's terms: six fp32 roundings, the rounded 1 / n among them), statistics within 1 ulp (exact sums, then a few
double roundings and one to fp32), dbias within 1 ulp + 2^-40 of its terms.  A dropped row, a flipped gate at z == 0, a wrong
group offset or a wrong ratio changes a sum by at least one unit.

Part B, derived bounds.  Real-valued data far from zero, with an outlier in row 0 (the shift), with a constant channel: mean, rstd
and the running statistics against worst-case any-order bounds of the shifted sums (tests/bn_cases.py: stat_bounds), the forward
output against the oracle evaluated with the kernel's own fp32 statistics.  Each prints `MEASURE name observed/bound`.

Every output is computed twice and must repeat its bits; outputs the caller provides (out of bn_fwd / bn_act_fwd / bn_fwd_grouped,
the in-place dy of bn_act_bwd / bn_act_bwd_grouped) lie in front of a guard row that must keep its sentinel -- the out-of-place dy of
bn_act_bwd and the dy of bn_act_bwd_conv1 are allocated by tg_hip.ops and have none.  The grouped forward computes its own
statistics, so its apply is exact on the m +- a data (even rows) and bounded at the returned statistics otherwise.
Not reached: the apply-stage grid cap of tg_bn_act_bwd_conv1 (more than 65536 * rlanes rows)."""
import numpy as np
import pytest
import torch

from tests import bn_cases as BC
from tests import bn_oracle as BO

pytestmark = pytest.mark.gpu

U = BO.U
EPS, MOM = BC.EPS32, BC.MOM32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def up(a, dev):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)       # a copy: never the builder's own memory


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def guarded(rows, C, dev, fill=None):
    """-> (buffer [rows + 1][C] whose last row is the sentinel, its first `rows` rows as the tensor to hand to an op)."""
    buf = torch.full((rows + 1, C), BC.SENTINEL, dtype=torch.float32, device=dev)
    if fill is not None:
        buf[:rows] = fill
    return buf, buf[:rows]


def guard_intact(buf):
    return bool((buf[-1] == BC.SENTINEL).all())


def same_bits(name, got, ref):
    """got (fp32, from the device) equals the float64 reference, which must itself be an fp32 number."""
    got, ref = np.asarray(got), np.asarray(ref, dtype=np.float64)
    assert got.dtype == np.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), f"{name}: the reference is not representable in fp32"
    bad = got.astype(np.float64) != ref
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[bad][0]!r} != {ref[bad][0]!r}"


def within(name, got, ref, tol, measure=False):
    """|got - ref| <= tol per element (tol == 0: equal); -> the largest observed / bound."""
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(tol, np.float64), np.shape(ref))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: not finite"
    diff = np.abs(got - ref)
    ratio = float(np.where(tol > 0, diff / np.where(tol > 0, tol, 1.0), np.where(diff > 0, np.inf, 0.0)).max()) if diff.size else 0.0
    if measure:
        print(f"MEASURE {name} {ratio:.4f}")
    assert ratio <= 1.0, f"{name}: observed / bound = {ratio:.4g} (worst |diff| {float(diff.max()):.3e}, relative {BO.err(got, ref):.3e})"
    return ratio


def one_ulp(name, got, ref):
    """Within 1 fp32 ulp of the rounded fp64 reference."""
    ref32 = np.asarray(ref, np.float64).astype(np.float32)
    return within(name, got, ref32.astype(np.float64), BO.ulp32(ref32))


def twice(fn):
    """Run fn() twice -> its first result (tuple of tensors / None), after asserting that the second has the same bits."""
    a, b = fn(), fn()
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        assert x is None or torch.equal(x, y), f"output {i} differs between two runs"
    return a


def check_backward(tag, got, ref, p_gamma, p_rstd, ratio, terms, rows, want_dbias, exact_dy):
    """got = (dy, dgamma, dbeta, dbias) from the device, ref = BO.bwd's tuple, terms = BO.bwd_terms' (|g|, |xh|)."""
    dy, dgamma, dbeta, dbias = (host(t) for t in got)
    rdy, rdgamma, rdbeta, rdbias, q = ref
    same_bits(f"{tag} dgamma", dgamma, rdgamma)
    same_bits(f"{tag} dbeta", dbeta, rdbeta)
    n = float(rows)
    gr = np.abs(np.asarray(p_gamma, np.float64) * np.asarray(p_rstd, np.float64))
    if exact_dy:
        same_bits(f"{tag} dy", dy.reshape(rdy.shape), rdy)
    else:
        rr = 1.0 if ratio is None else np.abs(np.asarray(ratio, np.float64))[:, None]
        absg, absxh = terms
        tol = 8 * U * gr * rr * (absg + np.abs(rdbeta) / n + absxh * np.abs(rdgamma) / n)
        within(f"{tag} dy", dy.reshape(rdy.shape), rdy, tol)
    if want_dbias:
        within(f"{tag} dbias", dbias, rdbias, dbias_tol(rdbias, gr, q, n))
    else:
        assert dbias is None


def dbias_tol(rdbias, gr, q, n):
    """1 fp32 ulp of the reference + 2^-40 |gamma rstd| (|q2| + |q0 q4| / n + |q1 q3| / n): the expression is evaluated in double and
    rounded once."""
    return BO.ulp32(rdbias) + 2.0 ** -40 * gr * (np.abs(q[2]) + np.abs(q[0] * q[4]) / n + np.abs(q[1] * q[3]) / n)


def pow2(n):
    return n & (n - 1) == 0


# ================================================================================================================================
# Part A: exact
# ================================================================================================================================
@pytest.mark.parametrize("case", BC.STAT_CASES, ids=BC.case_id)
def test_exact_statistics(dev, case):
    """tg_bn_stats and tg_bn_fwd (apply off; the one-launch kernel at the small shapes) on integer data: exact sums, so save_mean,
    save_rstd and the running statistics are within 1 ulp of the rounded oracle values; nbt counts one."""
    from tg_hip import ops as O
    rows, C = case
    o = BC.case_opts(BC.FWD_BWD_CASES, case)
    p = BC.exact_inputs(rows, C)
    y = up(p["y"], dev)
    mean, var, rstd = BO.stats(p["y"], EPS)
    rm0, rv0 = p["beta"], np.abs(p["gamma"])
    rrm, rrv = BO.running(rm0, rv0, mean, var, rows, MOM)

    def run(entry):
        rm, rv, nbt = (up(rm0, dev), up(rv0, dev), torch.full((), 5, dtype=torch.long, device=dev)) if o["running"] else (None, None, None)
        if entry == "bn_stats":
            m, r = O.bn_stats(y, rm, rv, nbt, eps=EPS, momentum=MOM)
        else:
            m, r, out = O.bn_fwd(y, up(p["gamma"], dev), up(p["beta"], dev), o["act"], BC.SLOPE, rm, rv, nbt, eps=EPS, momentum=MOM, apply=False)
            assert out is None
        return m, r, rm, rv, nbt

    for entry in ("bn_stats", "bn_fwd"):
        m, r, rm, rv, nbt = twice(lambda: run(entry))
        tag = f"{entry}[{BC.path(rows, C, entry)}] {rows}x{C}"
        one_ulp(f"{tag} mean", host(m), mean)
        one_ulp(f"{tag} rstd", host(r), rstd)
        if o["running"]:
            one_ulp(f"{tag} running_mean", host(rm), rrm)
            one_ulp(f"{tag} running_var", host(rv), rrv)
            assert int(nbt) == 6, int(nbt)


@pytest.mark.parametrize("case", BC.FWD_BWD_CASES, ids=BC.case_id)
def test_exact_forward_with_free_statistics(dev, case):
    """tg_bn_act_fwd (bn_act_fwd4_kernel / bn_act_fwd1_kernel) with free dyadic mean / rstd: the output bit for bit, z == 0 included."""
    from tg_hip import ops as O
    rows, C = case
    o = BC.case_opts(BC.FWD_BWD_CASES, case)
    p = BC.exact_inputs(rows, C)
    y, mean, rstd, gamma, beta = (up(p[k], dev) for k in ("y", "mean", "rstd", "gamma", "beta"))
    for act in (BC.ACTS if rows * C <= (1 << 20) else (o["act"],)):
        def run():
            buf, out = guarded(rows, C, dev)
            res = O.bn_act_fwd(y, mean, rstd, gamma, beta, act, BC.SLOPE, out=out)
            assert res.data_ptr() == buf.data_ptr() and guard_intact(buf)
            return (res.clone(),)
        (out,) = twice(run)
        ref = BO.apply(p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], act, BC.SLOPE)
        same_bits(f"bn_act_fwd {rows}x{C} {BC.ACT_NAME[act]}", host(out), ref)


@pytest.mark.parametrize("case", BC.FWD_BWD_CASES, ids=BC.case_id)
def test_exact_backward(dev, case):
    """tg_bn_act_bwd (first stage colreduce / colreduce4 / the one-launch kernel, finaliser, apply) with free dyadic statistics."""
    from tg_hip import ops as O
    rows, C = case
    o = BC.case_opts(BC.FWD_BWD_CASES, case)
    p = BC.exact_inputs(rows, C)
    ratio_h = p["ratio"] if o["ratio"] else None
    y, mean, rstd, gamma, beta, dout = (up(p[k], dev) for k in ("y", "mean", "rstd", "gamma", "beta", "dout"))
    ratio = up(ratio_h, dev)
    ref = BO.bwd(p["dout"], p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    terms = BO.bwd_terms(p["dout"], p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    tag = f"bn_act_bwd[{BC.path(rows, C, 'bn_act_bwd')}] {rows}x{C} {BC.ACT_NAME[o['act']]}"
    got = twice(lambda: O.bn_act_bwd(dout, y, mean, rstd, gamma, beta, o["act"], BC.SLOPE, ratio=ratio, inplace=False, want_dbias=o["dbias"]))
    assert torch.equal(dout, up(p["dout"], dev))                                   # out of place leaves dout alone
    check_backward(tag, got, ref, p["gamma"], p["rstd"], ratio_h, terms, rows, o["dbias"], pow2(rows))
    if o["inplace"]:
        buf, d = guarded(rows, C, dev, fill=dout)
        got2 = O.bn_act_bwd(d, y, mean, rstd, gamma, beta, o["act"], BC.SLOPE, ratio=ratio, inplace=True, want_dbias=o["dbias"])
        assert got2[0].data_ptr() == buf.data_ptr() and guard_intact(buf)
        for a, b in zip(got, got2):
            assert (a is None and b is None) or torch.equal(a, b), f"{tag}: in place differs from out of place"


EVEN = [c for c in BC.FWD_BWD_CASES if c[0] % 2 == 0]


@pytest.mark.parametrize("case", EVEN, ids=BC.case_id)
def test_dyadic_statistics_make_the_whole_chain_exact(dev, case):
    """Channels of m +- a in equal counts, eps = 0: mean == m and rstd == 1 / a exactly on every path (the one-launch kernel
    included), so tg_bn_fwd's output and the backward over its returned statistics are bit for bit."""
    from tg_hip import ops as O
    rows, C = case
    o = BC.case_opts(BC.FWD_BWD_CASES, case)
    p = BC.dyadic_stat_inputs(rows, C)
    ratio_h = p["ratio"] if o["ratio"] else None
    y, gamma, beta, dout = (up(p[k], dev) for k in ("y", "gamma", "beta", "dout"))
    rm0, rv0 = p["beta"], np.abs(p["gamma"])

    def fwd():
        rm, rv, nbt = (up(rm0, dev), up(rv0, dev), torch.zeros((), dtype=torch.long, device=dev)) if o["running"] else (None, None, None)
        buf, out = guarded(rows, C, dev)
        m, r, res = O.bn_fwd(y, gamma, beta, o["act"], BC.SLOPE, rm, rv, nbt, out=out, eps=0.0, momentum=MOM)
        assert res.data_ptr() == buf.data_ptr() and guard_intact(buf)
        return m, r, res.clone(), rm, rv, nbt

    m, r, out, rm, rv, nbt = twice(fwd)
    tag = f"bn_fwd[{BC.path(rows, C, 'bn_fwd')}] {rows}x{C} {BC.ACT_NAME[o['act']]}"
    same_bits(f"{tag} mean", host(m), p["m"])
    same_bits(f"{tag} rstd", host(r), 1.0 / p["a"].astype(np.float64))
    same_bits(f"{tag} out", host(out), BO.apply(p["y"], p["m"], 1.0 / p["a"], p["gamma"], p["beta"], o["act"], BC.SLOPE))
    if o["running"]:
        rrm, rrv = BO.running(rm0, rv0, p["m"], p["a"].astype(np.float64) ** 2, rows, MOM)
        one_ulp(f"{tag} running_mean", host(rm), rrm)
        one_ulp(f"{tag} running_var", host(rv), rrv)
        assert int(nbt) == 1
    ref = BO.bwd(p["dout"], p["y"], p["m"], 1.0 / p["a"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    terms = BO.bwd_terms(p["dout"], p["y"], p["m"], 1.0 / p["a"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    got = O.bn_act_bwd(dout, y, m, r, gamma, beta, o["act"], BC.SLOPE, ratio=up(ratio_h, dev), inplace=False, want_dbias=o["dbias"])
    check_backward(f"{tag} -> bn_act_bwd", got, ref, p["gamma"], 1.0 / p["a"], ratio_h, terms, rows, o["dbias"], pow2(rows))


@pytest.mark.parametrize("case", BC.CONV1_CASES, ids=BC.case_id)
def test_exact_backward_over_a_recomputed_1channel_dgrad(dev, case):
    """tg_bn_act_bwd_conv1: dz, w in {-1, 0, 1}, so the recomputed dout is an integer in [-9, 9] in both passes; share and non-share
    forms, H = 1 and W = 1 images, the first-stage grid cap.  (Its apply-stage cap needs more than 65536 * rlanes rows: left out.)"""
    from tg_hip import ops as O
    B, H, W, C = case
    rows = B * H * W
    o = BC.case_opts(BC.CONV1_CASES, case)
    p = BC.exact_conv1_inputs(B, H, W, C)
    ratio_h = p["ratio"] if o["ratio"] else None
    assert O.bn_bwd_conv1_supported((B, H, W, C))
    y = up(p["y"].reshape(B, H, W, C), dev)
    mean, rstd, gamma, beta, dz = (up(p[k], dev) for k in ("mean", "rstd", "gamma", "beta", "dz"))
    w = up(p["w"], dev).permute(2, 0, 1)[None]                                      # OIHW view of the [3][3][C] buffer
    ratio = None if ratio_h is None else up(ratio_h.reshape(B, H, W), dev)
    dout = BO.conv1_dgrad(p["dz"], p["w"]).reshape(rows, C)
    ref = BO.bwd(dout, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    terms = BO.bwd_terms(dout, p["y"], p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE, ratio_h)
    got = twice(lambda: O.bn_act_bwd_conv1(dz, w, y, mean, rstd, gamma, beta, o["act"], BC.SLOPE, ratio=ratio, want_dbias=o["dbias"]))
    g = BC.conv1_geom(rows, C)
    tag = f"bn_act_bwd_conv1[{'share' if g['share'] else 'plain'} qpp {g['qpp']}] {BC.case_id(case)} {BC.ACT_NAME[o['act']]}"
    check_backward(tag, got, ref, p["gamma"], p["rstd"], ratio_h, terms, rows, o["dbias"], pow2(rows))


@pytest.mark.parametrize("case", BC.GROUPED, ids=BC.case_id)
def test_exact_grouped(dev, case):
    """tg_bn_fwd_grouped / tg_bn_act_bwd_grouped: stacked passes with statistics per pass.  Forward on integer data (statistics
    within 1 ulp, the output against the oracle at the returned statistics within 5 * 2^-24 of its terms) and, where rows are even,
    on m +- a data (everything bit for bit); backward with free dyadic statistics that differ between the passes."""
    from tg_hip import ops as O
    rows_g, C, groups = case
    o = BC.case_opts(BC.GROUPED, case)
    p = BC.exact_grouped_inputs(rows_g, C, groups)
    gamma, beta = up(p["gamma"], dev), up(p["beta"], dev)
    tag = f"grouped {BC.case_id(case)} {BC.ACT_NAME[o['act']]}"

    def fwd(y):
        buf, out = guarded(groups * rows_g, C, dev)
        m, r, res = O.bn_fwd_grouped(y, groups, gamma, beta, o["act"], BC.SLOPE, out=out, eps=fwd.eps)
        assert res.data_ptr() == buf.data_ptr() and guard_intact(buf)
        return m, r, res.clone()

    fwd.eps = EPS
    m, r, out = (host(t) for t in twice(lambda: fwd(up(p["y"], dev))))
    mean, var, rstd = BO.stats_grouped(p["y"], groups, EPS)
    one_ulp(f"{tag} mean", m, mean)
    one_ulp(f"{tag} rstd", r, rstd)
    ref_out = BO.apply_grouped(p["y"], groups, m, r, p["gamma"], p["beta"], o["act"], BC.SLOPE)
    xh = np.concatenate([(p["y"][g * rows_g:(g + 1) * rows_g].astype(np.float64) - m[g]) * r[g] for g in range(groups)])
    within(f"{tag} out", out, ref_out, 5 * U * (np.abs(xh * p["gamma"]) + np.abs(p["beta"])))
    if rows_g % 2 == 0:
        d = [BC.dyadic_stat_inputs(rows_g, C, seed=g) for g in range(groups)]
        yd = np.concatenate([x["y"] for x in d])
        fwd.eps = 0.0
        m, r, out = (host(t) for t in twice(lambda: fwd(up(yd, dev))))
        dm, dr = np.stack([x["m"] for x in d]), np.stack([1.0 / x["a"].astype(np.float64) for x in d])
        same_bits(f"{tag} dyadic mean", m, dm)
        same_bits(f"{tag} dyadic rstd", r, dr)
        same_bits(f"{tag} dyadic out", out, BO.apply_grouped(yd, groups, dm, dr, p["gamma"], p["beta"], o["act"], BC.SLOPE))

    # backward, in place on dout
    y, mean_d, rstd_d = up(p["y"], dev), up(p["mean"], dev), up(p["rstd"], dev)

    def bwd():
        buf, dout = guarded(groups * rows_g, C, dev, fill=up(p["dout"], dev))
        dy, dg, db, dbi = O.bn_act_bwd_grouped(dout, y, groups, mean_d, rstd_d, gamma, beta, o["act"], BC.SLOPE, want_dbias=o["dbias"])
        assert dy.data_ptr() == buf.data_ptr() and guard_intact(buf)
        return dy.clone(), dg, db, dbi

    dy, dgamma, dbeta, dbias = (host(t) for t in twice(bwd))
    rdy, rdgamma, rdbeta, _, per = BO.bwd_grouped(p["dout"], p["y"], groups, p["mean"], p["rstd"], p["gamma"], p["beta"], o["act"], BC.SLOPE)
    same_bits(f"{tag} dgamma", dgamma, rdgamma)
    same_bits(f"{tag} dbeta", dbeta, rdbeta)
    n = float(rows_g)
    for g in range(groups):
        s = slice(g * rows_g, (g + 1) * rows_g)
        gr = np.abs(p["gamma"].astype(np.float64) * p["rstd"][g])
        if pow2(rows_g):
            same_bits(f"{tag} dy pass {g}", dy[s], rdy[s])
        else:
            absg, absxh = BO.bwd_terms(p["dout"][s], p["y"][s], p["mean"][g], p["rstd"][g], p["gamma"], p["beta"], o["act"], BC.SLOPE)
            within(f"{tag} dy pass {g}", dy[s], rdy[s], 8 * U * gr * (absg + np.abs(per[g][2]) / n + absxh * np.abs(per[g][1]) / n))
    if o["dbias"]:
        # every pass's term is rounded to fp32 (within t_g = dbias_tol of its exact value), the terms are added in fp32: against the
        # exact sum that is sum t_g + one rounding per addition, each at most an ulp at the size of sum |term| + sum t_g
        t = [dbias_tol(per[g][3], np.abs(p["gamma"].astype(np.float64) * p["rstd"][g]), per[g][4], n) for g in range(groups)]
        mag = sum(np.abs(per[g][3]) for g in range(groups)) + sum(t)
        within(f"{tag} dbias", dbias, sum(per[g][3] for g in range(groups)), sum(t) + (groups - 1) * BO.ulp32(mag))
    else:
        assert dbias is None


def _free_stats(C, groups=4):
    rng = np.random.default_rng(C)
    mean = rng.integers(-50, 51, (groups, C)).astype(np.float32)
    rstd = np.asarray((0.5, 1.0, 2.0), np.float32)[rng.integers(0, 3, (groups, C))]
    rm0, rv0 = (0.25 * rng.integers(-40, 41, C)).astype(np.float32), (0.25 * rng.integers(1, 41, C)).astype(np.float32)
    return mean, rstd, rm0, rv0


@pytest.mark.parametrize("C", [1, 12, 300])
@pytest.mark.parametrize("rows", [2, 683])
def test_running_update_from_saved_statistics(dev, C, rows):
    """tg_bn_running_update: the update tg_bn_stats would have made, from save_mean / save_rstd (var = 1 / rstd^2 - eps)."""
    from tg_hip import ops as O
    mean, rstd, rm0, rv0 = _free_stats(C)

    def run():
        rm, rv, nbt = up(rm0, dev), up(rv0, dev), torch.full((), 41, dtype=torch.long, device=dev)
        O.bn_running_update(up(mean[1], dev), up(rstd[1], dev), rows, rm, rv, nbt, eps=EPS, momentum=MOM)
        return rm, rv, nbt

    rm, rv, nbt = twice(run)
    rrm, rrv = BO.running(rm0, rv0, mean[1], BO.var_of_rstd(rstd[1], EPS), rows, MOM)
    one_ulp(f"running_update C={C} mean", host(rm), rrm)
    one_ulp(f"running_update C={C} var", host(rv), rrv)
    assert int(nbt) == 42


@pytest.mark.parametrize("C", [4, 300])
@pytest.mark.parametrize("order", BC.ORDERS, ids=lambda o: "".join(map(str, o)))
def test_running_update_multi_applies_the_passes_in_order(dev, C, order):
    from tg_hip import ops as O
    mean, rstd, rm0, rv0 = _free_stats(C)
    rows_g = 683

    def run():
        rm, rv, nbt = up(rm0, dev), up(rv0, dev), torch.full((), 7, dtype=torch.long, device=dev)
        O.bn_running_update_multi(up(mean, dev), up(rstd, dev), rows_g, order, rm, rv, nbt, eps=EPS, momentum=MOM)
        return rm, rv, nbt

    rm, rv, nbt = twice(run)
    rrm, rrv = BO.running_multi(rm0, rv0, mean, BO.var_of_rstd(rstd, EPS), rows_g, MOM, order)
    one_ulp(f"running_update_multi C={C} mean", host(rm), rrm)
    one_ulp(f"running_update_multi C={C} var", host(rv), rrv)
    assert int(nbt) == 7 + len(order)


# ================================================================================================================================
# Part B: derived bounds on real-valued data
# ================================================================================================================================
REAL = [(c, k) for c in BC.REAL_CASES for k in BC.REAL_KINDS]


@pytest.mark.parametrize("case,kind", REAL, ids=[f"{BC.case_id(c)}-{k}" for c, k in REAL])
def test_real_statistics_within_derived_bounds(dev, case, kind):
    """d = y - y[0], md = mean(d), u = 2^-24, all from the oracle:
    |mean - ref| <= (n + 2) u mean|d| + u |ref|;  |rstd - ref| / ref <= B_var / (var + eps) + 2 u with
    B_var = 2 (n + 8) u (mean(d^2) + md^2);  running var within momentum n / (n - 1) B_var + 1 ulp, running mean within momentum
    (n + 2) u mean|d| + 1 ulp (it is updated from the unrounded mean);  a constant channel: mean == y[0], rstd within 1 ulp of
    1 / sqrt(eps);  out against the oracle at the RETURNED fp32 mean / rstd within 5 u (|xh gamma| + |beta|) per element, which
    also covers an activation branch taken on the other side of a z within rounding of zero.
    scalar / quad: tg_bn_stats + tg_bn_act_fwd; small: tg_bn_fwd; grouped: tg_bn_fwd_grouped."""
    from tg_hip import ops as O
    pth, rows, C, groups = case
    act = BC.ACTS[(BC.REAL_CASES.index(case) + BC.REAL_KINDS.index(kind)) % 3]
    p = BC.real_inputs(kind, rows, C, groups)
    y, gamma, beta = up(p["y"], dev), up(p["gamma"], dev), up(p["beta"], dev)
    rng = np.random.default_rng(rows)
    rm0, rv0 = rng.standard_normal(C).astype(np.float32), (rng.random(C) + 0.5).astype(np.float32)

    def run():
        rm, rv, nbt = up(rm0, dev), up(rv0, dev), torch.zeros((), dtype=torch.long, device=dev)
        if pth == "grouped":
            m, r, out = O.bn_fwd_grouped(y, groups, gamma, beta, act, BC.REAL_SLOPE, eps=EPS)
            return m, r, out, None, None, None
        if pth == "small":
            m, r, out = O.bn_fwd(y, gamma, beta, act, BC.REAL_SLOPE, rm, rv, nbt, eps=EPS, momentum=MOM)
        else:
            m, r = O.bn_stats(y, rm, rv, nbt, eps=EPS, momentum=MOM)
            out = O.bn_act_fwd(y, m, r, gamma, beta, act, BC.REAL_SLOPE)
        return m, r, out, rm, rv, nbt

    assert BC.path(rows, C, "bn_fwd" if pth == "small" else "bn_stats") == ("quad" if pth == "grouped" else pth)
    m, r, out, rm, rv, nbt = (host(t) for t in twice(run))
    m, r = m.reshape(groups, C), r.reshape(groups, C)
    tag = f"{pth} {rows}x{C}" + (f"x{groups}" if groups > 1 else "") + f" {kind}"
    for g in range(groups):
        yg = p["y"][g * rows:(g + 1) * rows]
        b = BC.stat_bounds(yg, EPS)
        gt = tag + (f" pass {g}" if groups > 1 else "")
        within(f"{gt} mean", m[g], b["ref_mean"], b["mean"], measure=True)
        within(f"{gt} rstd", r[g] / b["rstd"], np.ones(C), b["rstd_rel"], measure=True)
        if rm is not None:
            rrm, rrv = BO.running(rm0, rv0, b["ref_mean"], b["var"], rows, MOM)
            within(f"{gt} running_mean", rm, rrm, MOM * b["mean_sum"] + BO.ulp32(rrm), measure=True)
            within(f"{gt} running_var", rv, rrv, MOM * rows / (rows - 1.0) * b["b_var"] + BO.ulp32(rrv), measure=True)
            assert int(nbt) == 1
        if kind == "const":
            c = p["const_channel"]
            assert m[g][c] == yg[0, c], (m[g][c], yg[0, c])
            one_ulp(f"{gt} constant channel rstd", r[g][c:c + 1], np.array([1.0 / np.sqrt(EPS)]))
        xh = (yg.astype(np.float64) - m[g]) * r[g]
        ref = BO.apply(yg, m[g], r[g], p["gamma"], p["beta"], act, BC.REAL_SLOPE)
        within(f"{gt} out", out.reshape(groups, rows, C)[g], ref, 5 * U * (np.abs(xh * p["gamma"]) + np.abs(p["beta"])), measure=True)
