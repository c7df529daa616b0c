"""GPU checks of test-time augmentation in inpaint_raster (csrc/raster.hip: tg_raster_gather_ops, tg_raster_tta_reduce,
tg_raster_blend_tta; mvp_gan/src/inpaint_raster.py) against the numpy mirrors in
tests/raster_tta_oracle.py: gather and reduce bit for bit, the blend bitwise in its raster and bounded in its spread, one
window against inpaint_batch, equivariance under the transforms, the known-pixel and unfilled-hole rules, evaluation and CLI."""
import json
import math

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO
from tests import raster_tta_oracle as TO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G(dev):
    from mvp_gan.src.models import PConvUNet
    torch.manual_seed(5)
    G = PConvUNet()
    g = torch.Generator().manual_seed(6)
    for m in G.modules():                       # non-trivial running statistics
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return G.to(dev)


def _cp(plan):
    from tg_hip import ops as O
    return O.raster_plan(plan.H, plan.W, plan.wh, plan.ww, plan.overlap, len(plan.ys), len(plan.xs))


def _bits(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a.view(np.int32)


def _tol(z, k):
    """The bound of tests/test_hip_raster.py: 1e-6 max|z| + 1e-6 range of the known heights."""
    zk = z[k].astype(np.float64)
    return 1e-6 * np.abs(zk).max() + 1e-6 * (zk.max() - zk.min())


def _d(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _gather_case(H, W):
    """The raster of test_stats_and_gather_bitwise where it fits: NaN, inf, nodata pixels, negative heights, an all-hole
    corner and a constant block with one hole."""
    z = RO.terrain(H, W, 11)
    z[:, 0] = -z[:, 0]
    mask = np.ones((H, W), np.float32)
    mask[:min(128, H), :128] = 0
    hole = RO.disc_holes(min(172, H), 132, 0.2, 12, 3, 10)
    mask[:hole.shape[0], :132][hole] = 0
    if H >= 300:
        z[172:, :128] = np.float32(431.25)
        mask[250, 60] = 0
        z[150, 200] = np.nan
        z[140, 100] = np.inf
        z[130, 50] = -9999.0
    else:
        z[50, 200] = np.nan
        z[40, 100] = np.inf
        z[30, 50] = -9999.0
    z[20, 200] = -9999.0
    return z, mask, -9999.0


@pytest.mark.parametrize("H,W,window,ops", [(300, 260, 128, TO.OPS), (100, 300, 128, (0, 1, 2, 3)), (300, 260, 72, TO.OPS)])
def test_gather_ops_bitwise(dev, H, W, window, ops):
    """Every window under every op in one call, against transform(RO.gather(...), op): tiles of exactly 64 (window 128), a
    partial tile row (100 x 128 windows) and a partial last tile both ways (72)."""
    from mvp_gan.src.inpaint_raster import plan_windows
    from tg_hip import ops as O
    plan = plan_windows(H, W, window, 16)
    assert (plan.wh, plan.ww) == (min(window, H), min(window, W))
    z, mask, nodata = _gather_case(H, W)
    zd, md = _d(z, dev), _d(mask, dev)
    lo, hi, cnt = O.raster_window_stats(zd, md, _cp(plan), nodata)
    rlo, rhi, rcnt = RO.stats(z, plan, mask, nodata)
    np.testing.assert_array_equal(cnt.cpu().numpy(), rcnt)
    np.testing.assert_array_equal(_bits(lo.cpu().numpy()), _bits(rlo))
    np.testing.assert_array_equal(_bits(hi.cpu().numpy()), _bits(rhi))
    nwin = len(plan.ys) * len(plan.xs)
    wins = np.repeat(np.arange(nwin, dtype=np.int32)[::-1], len(ops))          # any window order
    opi = np.tile(np.array(ops, np.int32), nwin)
    x, m = O.raster_gather_ops(zd, md, _cp(plan), lo, hi, _d(wins, dev), opi, nodata)
    rx, rm = RO.gather(z, plan, rlo, rhi, wins, mask, nodata)
    assert x.shape == m.shape == (wins.size, plan.wh, plan.ww)
    gx, gm = x.cpu().numpy(), m.cpu().numpy()
    for k in range(wins.size):
        np.testing.assert_array_equal(_bits(gx[k]), _bits(TO.transform(rx[k], opi[k])), err_msg=f"item {k} op {opi[k]}")
        np.testing.assert_array_equal(gm[k], TO.transform(rm[k], opi[k]), err_msg=f"item {k} op {opi[k]}")
    # op 0 is tg_raster_gather, bit for bit
    idx = _d(np.arange(nwin, dtype=np.int32), dev)
    x0, m0 = O.raster_gather(zd, md, _cp(plan), lo, hi, idx, nodata)
    x1, m1 = O.raster_gather_ops(zd, md, _cp(plan), lo, hi, idx, np.zeros(nwin, np.int32), nodata)
    assert torch.equal(x0.view(torch.int32), x1.view(torch.int32)) and torch.equal(m0, m1)
    if plan.wh != plan.ww:
        from tg_hip import lib as L
        with pytest.raises(L.TgError, match="square"):
            O.raster_gather_ops(zd, md, _cp(plan), lo, hi, idx, np.full(nwin, 4, np.int32), nodata)


VAR_EXACT = {2: np.float32(0.5), 4: np.float32(5) / np.float32(3), 8: np.float32(6)}


@pytest.mark.parametrize("wh,ww,T", [(72, 72, 2), (72, 72, 4), (72, 72, 8), (100, 128, 2), (100, 128, 4)])
def test_reduce_exact_and_bitwise(dev, wh, ww, T):
    """Integer frames base + t under op_t: the mean is base + (T - 1) / 2 and the variance 0.5, 5/3 or 6 exactly, and a wrong
    inverse of any op moves pixels; then random frames (three windows) bitwise against the float32 mirror."""
    from tg_hip import ops as O
    ops = TO.OPS[:T]
    base = np.arange(wh * ww, dtype=np.float32).reshape(wh, ww)
    g = np.stack([TO.transform(base, op) + np.float32(t) for t, op in enumerate(ops)])[None]
    mean, var = O.raster_tta_reduce(_d(g, dev), np.array(ops, np.int32))
    np.testing.assert_array_equal(mean.cpu().numpy()[0], base + np.float32((T - 1) / 2))
    np.testing.assert_array_equal(var.cpu().numpy()[0], np.full((wh, ww), VAR_EXACT[T]))
    rng = np.random.default_rng(100 * T + wh)
    g = rng.random((3, T, wh, ww)).astype(np.float32)
    g[1, 0, 5, 7] = np.nan
    for member_ops in (ops, ops[::-1]):
        mean, var = O.raster_tta_reduce(_d(g, dev), np.array(member_ops, np.int32))
        rmean, rvar = TO.reduce(g, member_ops)
        np.testing.assert_array_equal(_bits(mean.cpu().numpy()), _bits(rmean))
        np.testing.assert_array_equal(_bits(var.cpu().numpy()), _bits(rvar))
    if wh != ww:
        from tg_hip import lib as L
        with pytest.raises(L.TgError, match="square"):
            O.raster_tta_reduce(_d(g[:, :2], dev), np.array((0, 4), np.int32))


def test_blend_tta_against_float64(dev):
    """The inputs of test_blend_against_float64 with random window means in [0, 1) and variances in [0, 0.01).

    The raster and the unfilled count are bitwise tg_raster_blend's.  Bound on the spread: it is the weighted L2 norm
    sqrt(sum_j w_j c_j^2 / sum_j w_j) of the components sqrt(var_j) d_j and dn_j - out, so by the triangle inequality it moves
    by no more than the largest component error.  dn_j and out each carry a few ulp of max|z| in fp32 (the _tol of
    tests/test_hip_raster.py: 1e-6 max|z| + 1e-6 range, which bounds out against float64), and var_j d_j^2 a relative error
    of a few ulp; the fp32 accumulation over at most four windows and the square root add a relative error of a few 2^-24,
    covered by 1e-6 ref.  Hence |spread - ref| <= 1e-6 max|z| + 1e-6 range + 1e-6 ref."""
    from mvp_gan.src.inpaint_raster import plan_windows
    from tg_hip import ops as O
    H, W = 1500, 2100
    plan = plan_windows(H, W, 512, 64)
    nwin = len(plan.ys) * len(plan.xs)
    z = RO.terrain(H, W, 21)
    hole = RO.disc_holes(H, W, 0.3, 22, 10, 60)
    mask = (~hole).astype(np.float32)
    zd, md = _d(z, dev), _d(mask, dev)
    lo, hi, cnt = O.raster_window_stats(zd, md, _cp(plan))
    rng = np.random.default_rng(23)
    run_of = np.full(nwin, -1, np.int32)
    ran = np.sort(rng.choice(nwin, nwin - 3, replace=False))   # three windows did not run
    run_of[ran] = rng.permutation(ran.size)                     # any row order of the output buffer
    wmean = rng.random((ran.size, plan.wh, plan.ww)).astype(np.float32)
    wvar = (rng.random((ran.size, plan.wh, plan.ww)) * 0.01).astype(np.float32)
    args = (zd, md, _cp(plan), lo, hi, _d(run_of, dev), _d(wmean, dev))
    out, spread, unfilled = O.raster_blend_tta(*args, _d(wvar, dev))
    out0, unfilled0 = O.raster_blend(*args)
    assert torch.equal(out.view(torch.int32), out0.view(torch.int32)) and int(unfilled.item()) == int(unfilled0.item())
    ref, rspread, runf = TO.blend_tta(z, plan, lo.cpu().numpy(), hi.cpu().numpy(), run_of, wmean, wvar, mask)
    got = spread.cpu().numpy()
    k = mask != 0
    assert int(unfilled.item()) == runf and runf > 0
    assert (got[k] == 0).all() and not np.signbit(got[k]).any()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(rspread))
    np.testing.assert_array_equal(np.isnan(got), np.isnan(out.cpu().numpy()))
    f = ~k & ~np.isnan(rspread)
    err = np.abs(got[f] - rspread[f])
    bound = _tol(z, k) + 1e-6 * rspread[f]
    print(f"spread: max err {err.max():.3e} m, smallest bound {bound.min():.3e} m, largest err / bound {(err / bound).max():.3f}, "
          f"spread range {rspread[f].min():.3g} .. {rspread[f].max():.3g} m")
    assert (err <= bound).all(), (err.max(), (err / bound).max())
    out2, spread2, _ = O.raster_blend_tta(*args, _d(wvar, dev))
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    assert torch.equal(spread2.view(torch.int32), spread.view(torch.int32))


@pytest.fixture(scope="module")
def one_window():
    z = RO.terrain(128, 128, 81)
    mask = (~RO.disc_holes(128, 128, 0.3, 82, 5, 20)).astype(np.float32)
    return z, mask


def test_single_window_matches_inpaint_batch(dev, G, one_window):
    """One 128 x 128 window, tta=8: the eight numpy-transformed (x, m) through inpaint_batch, inverted, float64 mean and sample
    standard deviation.  The mean agrees within 1e-6 (hi - lo), the bound of tests/test_hip_raster.py's single-window test; the
    spread within four times that: a standard deviation is an L2 norm of the member deviations, which a member error delta moves
    by at most about 2 delta sqrt(T / (T - 1))."""
    from mvp_gan.src.evaluate import inpaint_batch
    from mvp_gan.src.inpaint_raster import inpaint_raster_tta, plan_windows
    z, mask = one_window
    was = G.training
    out, spread, info = inpaint_raster_tta(G, z, mask, window=128, overlap=16)
    assert G.training == was
    assert info["windows"] == 1 and info["run"] == 1 and info["unfilled"] == 0 and info["tta"]["members"] == 8
    plan = plan_windows(128, 128, 128, 16)
    lo, hi, _ = RO.stats(z, plan, mask)
    x, m = RO.gather(z, plan, lo, hi, [0], mask)
    xs = np.stack([TO.transform(x[0], op) for op in TO.OPS])[:, None]
    ms = np.stack([TO.transform(m[0], op) for op in TO.OPS])[:, None]
    o = inpaint_batch(G, _d(xs, dev), _d(ms, dev)).cpu().numpy()[:, 0].astype(np.float64)
    o = np.stack([TO.inverse(o[t], op) for t, op in enumerate(TO.OPS)])
    rng_ = float(hi[0]) - float(lo[0])
    k = mask != 0
    ref = np.where(k, z, float(lo[0]) + o.mean(0) * rng_)
    rsp = np.where(k, 0.0, o.std(0, ddof=1) * rng_)
    got, gsp = out.cpu().numpy(), spread.cpu().numpy()
    assert out.dtype == spread.dtype == torch.float32 and out.is_cuda and spread.is_cuda and got.shape == gsp.shape == (128, 128)
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    err, serr = np.abs(got - ref).max(), np.abs(gsp - rsp).max()
    print(f"mean err {err:.3e} m, spread err {serr:.3e} m, bound {1e-6 * rng_:.3e} m, spread up to {rsp.max():.3g} m")
    assert err <= 1e-6 * rng_, (err, 1e-6 * rng_)
    assert serr <= 4e-6 * rng_, (serr, 4e-6 * rng_)
    holes = ~k
    assert info["tta"]["max_spread_m"] == float(gsp[holes].max())
    assert abs(info["tta"]["mean_spread_m"] - float(gsp[holes].astype(np.float64).mean())) <= 1e-9 * rsp.max()
    json.dumps(info)


def test_equivariance(dev, G, one_window):
    """The eight-member ensemble of a transformed raster, mapped back, is the ensemble of the raster: both runs feed the
    generator the same eight inputs in another order, which _tol (what test_determinism_and_batch_size allows for a different
    batch composition) covers, four times that for the spread.  With one member the same comparison must fail: the randomly
    initialised generator is not symmetric (on the CPU oracle: 6e3 to 8e3 times the bound, tests/test_raster_tta_cpu.py)."""
    from mvp_gan.src.inpaint_raster import inpaint_raster, inpaint_raster_tta
    z, mask = one_window
    k = mask != 0
    tol = _tol(z, k)
    a, sa, _ = inpaint_raster_tta(G, z, mask, window=128, overlap=16)
    a1, _ = inpaint_raster(G, z, mask, window=128, overlap=16, tta=1)
    a, sa, a1 = a.cpu().numpy().astype(np.float64), sa.cpu().numpy().astype(np.float64), a1.cpu().numpy().astype(np.float64)
    for op in (1, 4, 7):
        zt, mt = TO.transform(z, op), TO.transform(mask, op)
        b, sb, _ = inpaint_raster_tta(G, zt, mt, window=128, overlap=16)
        err = np.abs(TO.inverse(b.cpu().numpy(), op) - a).max()
        serr = np.abs(TO.inverse(sb.cpu().numpy(), op) - sa).max()
        b1, _ = inpaint_raster(G, zt, mt, window=128, overlap=16, tta=1)
        err1 = np.abs(TO.inverse(b1.cpu().numpy(), op) - a1).max()
        print(f"op {op}: mean {err:.3e} m, spread {serr:.3e} m, tol {tol:.3e} m; tta=1 {err1:.3e} m = {err1 / tol:.3g} x tol")
        assert err <= tol, (op, err, tol)
        assert serr <= 4 * tol, (op, serr, 4 * tol)
        assert err1 > tol, (op, err1, tol)


def test_rules(dev, G):
    """Known pixels bit for bit with spread 0; the unfilled count and the NaN set of tta=1, NaN in the spread there; repeats
    bitwise; inpaint_raster(tta=4) is inpaint_raster_tta's first output; tta=1 is the default path; non-square windows."""
    from mvp_gan.src.inpaint_raster import inpaint_raster, inpaint_raster_tta
    H, W = 600, 640
    z = RO.terrain(H, W, 41)
    mask = (~RO.disc_holes(H, W, 0.15, 42, 5, 20)).astype(np.float32)
    mask[:256, :256] = 0                                        # window (0,0) has no known pixel: it does not run
    z[400, 500] = np.nan
    z[410, 30] = -32768.0
    zd, md = _d(z, dev), _d(mask, dev)
    kw = dict(nodata=-32768.0, window=256, overlap=32, batch=4)
    out, spread, info = inpaint_raster_tta(G, zd, md, tta=4, **kw)
    base, binfo = inpaint_raster(G, zd, md, **kw)
    got, gsp, gb = out.cpu().numpy(), spread.cpu().numpy(), base.cpu().numpy()
    k = RO.known(z, mask, -32768.0)
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    assert (gsp[k] == 0).all()
    only00 = np.zeros((H, W), bool)
    only00[:224, :224] = True                                   # covered by window (0,0) alone
    np.testing.assert_array_equal(np.isnan(got), only00)
    np.testing.assert_array_equal(np.isnan(gb), only00)
    np.testing.assert_array_equal(np.isnan(gsp), only00)
    assert info["unfilled"] == binfo["unfilled"] == 224 * 224
    assert {kk: v for kk, v in info.items() if kk != "tta"} == binfo and "tta" not in binfo
    assert info["tta"]["members"] == 4 and 0 < info["tta"]["mean_spread_m"] <= info["tta"]["max_spread_m"] < math.inf
    assert (gsp[~k & ~only00] >= 0).all()
    out2, spread2, info2 = inpaint_raster_tta(G, zd, md, tta=4, **kw)
    assert info2 == info
    np.testing.assert_array_equal(_bits(out2.cpu().numpy()), _bits(got))
    np.testing.assert_array_equal(_bits(spread2.cpu().numpy()), _bits(gsp))
    out3, info3 = inpaint_raster(G, zd, md, tta=4, **kw)
    assert info3 == info
    np.testing.assert_array_equal(_bits(out3.cpu().numpy()), _bits(got))
    base1, binfo1 = inpaint_raster(G, zd, md, tta=1, **kw)
    assert binfo1 == binfo
    np.testing.assert_array_equal(_bits(base1.cpu().numpy()), _bits(gb))
    # 100 x 128 windows: the four plain members
    z2 = RO.terrain(100, 300, 43)
    mask2 = (~RO.disc_holes(100, 300, 0.2, 44, 3, 10)).astype(np.float32)
    o2, s2, i2 = inpaint_raster_tta(G, z2, mask2, tta=4, window=128, overlap=16)
    k2 = mask2 != 0
    g2, gs2 = o2.cpu().numpy(), s2.cpu().numpy()
    np.testing.assert_array_equal(_bits(g2[k2]), _bits(z2[k2]))
    assert i2["windows"] == 3 and i2["unfilled"] == 0 and np.isfinite(g2).all() and (gs2[k2] == 0).all() and (gs2[~k2] >= 0).all() and gs2.max() > 0
    with pytest.raises(ValueError, match="tta=4"):
        inpaint_raster_tta(G, z2, mask2, window=128, overlap=16)


def test_model_cellsize_spread_on_native_grid(dev, G):
    """With a working grid the spread returns to the native grid like the mean: the raster's shape, 0 at the native known
    pixels, finite at the holes; the mean is inpaint_raster's, and the seam correction leaves the spread alone."""
    from mvp_gan.src.inpaint_raster import inpaint_raster, inpaint_raster_tta
    H, W = 160, 200
    z = RO.terrain(H, W, 91)
    mask = (~RO.disc_holes(H, W, 0.2, 92, 4, 12)).astype(np.float32)
    z[10, 20] = np.nan
    kw = dict(cellsize=1.0, model_cellsize=2.0, window=64, overlap=16, batch=4)
    out, spread, info = inpaint_raster_tta(G, z, mask, tta=2, **kw)
    ref, rinfo = inpaint_raster(G, z, mask, tta=2, **kw)
    assert info == rinfo and info["resample"]["shape"] == (80, 100) and info["tta"]["members"] == 2
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    k = RO.known(z, mask)
    got, gsp = out.cpu().numpy(), spread.cpu().numpy()
    assert gsp.shape == (H, W) and spread.dtype == torch.float32
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    assert (gsp[k] == 0).all() and np.isfinite(gsp[~k]).all() and (gsp[~k] >= 0).all() and gsp.max() > 0
    assert info["tta"]["max_spread_m"] == float(gsp[~k].max())
    out2, spread2, info2 = inpaint_raster_tta(G, z, mask, tta=2, seam="harmonic", **kw)
    assert "seam" in info2 and torch.equal(spread2.view(torch.int32), spread.view(torch.int32))


def test_evaluate_raster_spread_row(dev, G):
    """evaluate_raster(tta=2) at the geometry of test_evaluate_raster_end_to_end: the report gains "spread" with a calibration
    over the scored holes, stays JSON-serialisable, and the prediction is inpaint_raster(tta=2)'s; without tta no such key."""
    from mvp_gan.src.evaluate_raster import calibration_summary, eval_holes, evaluate_raster
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H, W, c = 1500, 2100, 2.0
    z = RO.terrain(H, W, 4, base=200.0, relief=60.0)
    z[700:720, 100:200] = np.nan
    kw = dict(cellsize=c, split="test", block=512, tile=128, seed=2, window=256, overlap=32, batch=8)
    rep, pred = evaluate_raster(G, z, tta=2, **kw)
    sp = rep["spread"]
    assert sorted(sp) == ["calibration", "max_m", "mean_m", "members"] and sp["members"] == 2
    assert sp["calibration"]["cells"] > 0 and sp["calibration"]["cells"] <= rep["pixels"]["scored"]
    assert math.isfinite(sp["mean_m"]) and math.isfinite(sp["max_m"]) and 0 < sp["mean_m"] <= sp["max_m"]
    assert math.isfinite(sp["calibration"]["mean_z2"]) and "calibration" in calibration_summary(sp["calibration"])
    assert rep["inpaint"]["tta"] == {"members": 2, "mean_spread_m": sp["mean_m"], "max_spread_m": sp["max_m"]}
    json.loads(json.dumps(rep))
    _, keep, _ = eval_holes(z, split="test", block=512, tile=128, seed=2)
    ref_pred, _ = inpaint_raster(G, z, keep, window=256, overlap=32, batch=8, tta=2)
    assert torch.equal(pred.view(torch.int32), ref_pred.view(torch.int32))
    rep1, _ = evaluate_raster(G, z, **kw)
    assert "spread" not in rep1 and "tta" not in rep1["inpaint"]


def test_cli_spread_out(dev, G, tmp_path, capsys):
    from mvp_gan.src.asc import read_asc, write_asc
    from mvp_gan.src.inpaint_raster import main
    H, W = 120, 100
    z = RO.terrain(H, W, 71)
    z[RO.disc_holes(H, W, 0.2, 72, 3, 8)] = -9999.0
    hdr = [("ncols", str(W)), ("nrows", str(H)), ("xllcorner", "400000.0"), ("yllcorner", "300000.0"), ("cellsize", "2"),
           ("NODATA_value", "-9999")]
    write_asc(tmp_path / "in.asc", z, hdr)
    torch.save({"generator_state_dict": G.state_dict()}, tmp_path / "g.pth")
    info = main(["--dem", str(tmp_path / "in.asc"), "--checkpoint", str(tmp_path / "g.pth"), "--out", str(tmp_path / "out.asc"),
                 "--window", "64", "--overlap", "16", "--batch", "3", "--tta", "2", "--spread-out", str(tmp_path / "s.asc")])
    assert info["windows"] == 6 and info["run"] == 6 and info["unfilled"] == 0 and info["tta"]["members"] == 2
    assert "tta 2: spread" in capsys.readouterr().out
    got, hdr2 = read_asc(tmp_path / "out.asc")
    s, hdr3 = read_asc(tmp_path / "s.asc")
    assert hdr2 == hdr and hdr3 == hdr and s.shape == got.shape == (H, W)
    k = z != -9999.0
    np.testing.assert_array_equal(_bits(got[k]), _bits(z[k]))
    assert (s[k] == 0).all() and (s[~k] >= 0).all() and s.max() > 0 and np.isfinite(s).all() and np.isfinite(got).all()
    assert info["tta"]["max_spread_m"] == pytest.approx(float(s.max()), rel=1e-6)
