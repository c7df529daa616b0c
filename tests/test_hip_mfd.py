"""GPU checks of the multiple-flow-direction accumulation, the slope and the wetness index (csrc/mfd.hip,
mvp_gan/src/flow_routing.py) against the numpy oracle of tests/mfd_oracle.py.

The float64 plane, the float32 accumulation, the three class counts and the largest value are compared bit for bit; mass_out is
held to 1e-12 relative against the number of known pixels.  The slope is compared bit for bit with the oracle's float32
restatement, NaN pattern included (the bound was 2 ulp, since sqrtf is documented at 1 ulp; on the MI355X every pixel of every
scene came out bitwise equal, so the test asks for that); the wetness index to
2^-21 + 2^-22 |ref| of the float64 logarithm of the oracle's float32 operands (three ulp of the ratio, logf at its documented
1 ulp, the final rounding); the comparison kernel's count and maximum exactly, its sums to 1e-12 relative."""
import json

import numpy as np
import pytest
import torch

from tests import flow_oracle as FO
from tests import mfd_oracle as MO

pytestmark = pytest.mark.gpu
MASS_RTOL = 1e-12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _ops_plane(dev, w, known, direction, e, check_every=8):
    """mfd_known on uploaded arrays -> (acc float32, A float64, info), as numpy."""
    from mvp_gan.src.flow_routing import mfd_known
    wt = torch.from_numpy(np.array(w, np.float32)).to(dev)
    kt = torch.from_numpy(np.asarray(known).astype(np.uint8)).to(dev)
    dt = torch.from_numpy(np.array(direction, np.uint8)).to(dev)
    acc, A, info = mfd_known(wt, kt, dt, exponent=e, check_every=check_every)
    assert acc.dtype == torch.float32 and A.dtype == torch.float64
    return acc.cpu().numpy(), A.cpu().numpy(), info


def _against(m, known, acc, A, info, what):
    """One result against the oracle's dict m: bits of both planes, counts, maximum, mass."""
    n = int(np.asarray(known, bool).sum())
    print(what, {k: info[k] for k in ("dispersive", "single", "sinks", "mfd_sweeps", "mfd_tile_visits", "max_accumulation_mfd",
                                      "mass_out")}, "mass err", abs(info["mass_out"] - n) / max(n, 1))
    if A is not None:
        bad = np.nonzero(_bits(A) != _bits(m["A"]))
        assert not bad[0].size, (what, bad[0].size, bad[0][:4], bad[1][:4], A[bad][:4], m["A"][bad][:4])
    np.testing.assert_array_equal(_bits(acc), _bits(m["acc"]), err_msg=what)
    assert {k: info[k] for k in ("dispersive", "single", "sinks")} == m["counts"], what
    assert info["max_accumulation_mfd"] == m["max"], what
    assert abs(info["mass_out"] - n) <= MASS_RTOL * n, (what, info["mass_out"], n)
    assert info["mfd_sweeps"] >= 1 and info["mfd_tile_visits"] >= 1 or n == 0


# ---- the scenes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", MO.EXPONENTS)
@pytest.mark.parametrize("name", list(MO.scenes()))
def test_scenes(dev, name, e):
    """mfd_accumulation end to end, and the float64 plane through the ops on the oracle's routing."""
    from mvp_gan.src.flow_routing import mfd_accumulation
    z, nodata, fill, r, m = MO.scene_ref(name, e)
    acc, info = mfd_accumulation(z, nodata=nodata, cellsize=2.0, fill=fill, exponent=e)
    assert acc.dtype == torch.float32 and tuple(acc.shape) == z.shape
    assert info["exponent"] == e and info["known"] == int(r["known"].sum()) and info["converged"] and info["filled"] is fill
    _against(m, r["known"], acc.cpu().numpy(), None, info, f"{name} e={e} end to end")
    acc2, A, info2 = _ops_plane(dev, r["w"], r["known"], r["dir"], e)
    _against(m, r["known"], acc2, A, info2, f"{name} e={e} ops")
    if name == "serpentine":
        assert info2["mfd_sweeps"] > 8                              # 8256 steps: the inner-round cap is hit, the tiles stay listed


@pytest.mark.parametrize("shape", ((1, 1), (1, 77), (77, 1), (63, 65), (64, 64), (65, 193), (193, 65)))
def test_shapes(dev, shape):
    from mvp_gan.src.flow_routing import mfd_accumulation
    H, W = shape
    z = FO.rounded_pits(H, W, 10 * H + W, npits=min(6, H * W))
    for fill in (True, False):
        r = FO.route(z, fill=fill)
        for e in MO.EXPONENTS:
            m = MO.mfd(r["w"], r["known"], r["dir"], e)
            acc, info = mfd_accumulation(z, fill=fill, exponent=e)
            _against(m, r["known"], acc.cpu().numpy(), None, info, f"{H}x{W} fill={fill} e={e}")
            acc2, A, info2 = _ops_plane(dev, r["w"], r["known"], r["dir"], e)
            _against(m, r["known"], acc2, A, info2, f"{H}x{W} fill={fill} e={e} ops")
    if shape == (1, 1):
        assert acc.cpu().tolist() == [[1.0]] and info["sinks"] == 1 and info["mass_out"] == 1.0


def test_unconverged_fill_leaves_nan(dev):
    """max_sweeps = 1: the fill has not reached the inner tile, w holds NaN there; such a pixel is never a valid drop, gives
    nothing and receives nothing.  The oracle gets the surface and the directions the GPU routed."""
    from mvp_gan.src.flow_routing import mfd_known, route_raster
    from tests import depfill_oracle as DO
    z = DO.pits_scene(192, 192, 21)
    direction, _, info, w = route_raster(z, None, None, 1.0, True, 1, 1, "test")
    wn, dn = w.cpu().numpy(), direction.cpu().numpy()
    nan = np.isnan(wn)
    assert not info["converged"] and nan.sum() > 1000 and (dn != 0).all()
    known = np.ones(z.shape, bool)
    kt = torch.ones(z.shape, dtype=torch.uint8, device=dev)
    for e in (1, 4):
        m = MO.mfd(wn, known, dn, e)
        acc, A, minfo = mfd_known(w, kt, direction, exponent=e)
        _against(m, known, acc.cpu().numpy(), A.cpu().numpy(), minfo, f"unconverged e={e}")
        assert (A.cpu().numpy()[nan] == 1.0).all() and (m["cls"][nan] == MO.SINK).all()


# ---- schedule independence ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("serpentine", "rounded", "spiral"))
def test_reproducible_and_check_every(dev, name):
    z, nodata, fill, r, m = MO.scene_ref(name, 1)
    planes = []
    for ce in (1, 8, 1, 8):
        acc, A, info = _ops_plane(dev, r["w"], r["known"], r["dir"], 1, check_every=ce)
        assert info["mfd_sweeps"] >= 1 and info["mfd_tile_visits"] >= 1
        assert info["mfd_sweeps"] % ce == 0
        print(name, "check_every", ce, info["mfd_sweeps"], "sweeps", info["mfd_tile_visits"], "visits")
        planes.append((A, acc, info["mass_out"], info["max_accumulation_mfd"]))
    for A, acc, mass, amax in planes:
        assert np.array_equal(_bits(A), _bits(planes[0][0])) and np.array_equal(_bits(acc), _bits(planes[0][1]))
        assert mass == planes[0][2] and amax == planes[0][3]
    assert np.array_equal(_bits(planes[0][0]), _bits(m["A"]))


# ---- slope and wetness -------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """Distance in float32 steps between finite arrays of one sign pattern."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("name,c", (("void", 2.0), ("rounded", 0.5), ("pits", 30.0)))
def test_slope(dev, name, c):
    from mvp_gan.src.flow_routing import terrain_slope
    z, nodata, fill, r, m = MO.scene_ref(name, 1)
    got = terrain_slope(z, nodata=nodata, cellsize=c)
    assert got.dtype == torch.float32
    got = got.cpu().numpy()
    known = r["known"]
    want = MO.slope(np.where(known, z, np.float32(0)), known, c)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got), ~known)
    u = _ulps(got[known], want[known])
    print(name, "slope ulp max", int(u.max()), "differing", int((u > 0).sum()), "of", int(known.sum()))
    assert u.max() == 0                                             # tightened from 2 ulp: sqrtf comes out correctly rounded
    assert (got[known] >= 0).all()


@pytest.mark.parametrize("name,e,c,ms", (("void", 1, 2.0, 1e-3), ("pits", 4, 1.0, 1e-3), ("lake", 8, 30.0, 0.05)))
def test_wetness_index(dev, name, e, c, ms):
    from mvp_gan.src.flow_routing import wetness_index
    z, nodata, fill, r, m = MO.scene_ref(name, e)
    twi, acc, slope, info = wetness_index(z, nodata=nodata, cellsize=c, fill=fill, exponent=e, min_slope=ms)
    known = r["known"]
    twi, acc, slope = twi.cpu().numpy(), acc.cpu().numpy(), slope.cpu().numpy()
    assert twi.dtype == np.float32 and info["min_slope"] == ms and info["exponent"] == e
    np.testing.assert_array_equal(_bits(acc), _bits(m["acc"]))
    want_slope = MO.slope(r["w"], known, c)
    assert np.array_equal(np.isnan(slope), ~known) and _ulps(slope[known], want_slope[known]).max() == 0
    ref = MO.twi_ref(m["acc"], want_slope, known, c, ms)
    assert np.array_equal(np.isnan(twi), ~known) and np.isfinite(twi[known]).all()
    err = np.abs(twi[known].astype(np.float64) - ref[known])
    bound = MO.twi_bound(ref[known])
    print(name, "twi worst err / bound", float((err / bound).max()), "range", float(ref[known].min()), float(ref[known].max()))
    assert (err <= bound).all()
    if ms == 0.05:
        assert (slope[known] < ms).any()                            # the lake: the floor of the slope is in use


def test_wetness_compare_kernel(dev):
    from tg_hip import ops as O
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (77, 130), (300, 517)):
        t = rng.normal(6, 3, (H, W)).astype(np.float32)
        p = (t + rng.normal(0, 1, (H, W))).astype(np.float32)
        sel = (rng.random((H, W)) < 0.4).astype(np.uint8)
        for a in (t, p):
            a[rng.random((H, W)) < 0.03] = np.nan
            a[rng.random((H, W)) < 0.01] = np.inf
            a[rng.random((H, W)) < 0.01] = -np.inf
        want = MO.wetness_stats(sel, t, p)
        runs = []
        for _ in range(2):
            counts, sums = O.wetness_compare(torch.from_numpy(sel).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev))
            runs.append((counts.cpu().tolist(), sums.cpu().tolist()))
        assert runs[0] == runs[1]                                   # a fixed order: bitwise reproducible
        (cells, bits), sums = runs[0]
        assert cells == want[0] and np.array([bits], np.uint32).view(np.float32)[0] == want[4]
        for got, ref in zip(sums, want[1:4]):
            assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
        if cells == 0:
            assert sums == [0.0, 0.0, 0.0] and bits == 0


def test_wetness_errors(dev):
    """wetness_errors against the same comparison of two wetness_known planes made here, its count and maximum exactly, each of
    its three sums (wetness_raw) to 1e-12 relative against numpy, as the comparison kernel's."""
    from mvp_gan.src.evaluate_raster import wetness_errors, wetness_raw
    from mvp_gan.src.flow_routing import wetness_known
    rng = np.random.default_rng(9)
    z = MO.scenes()["pits"][0].copy()
    z[5, 7] = np.nan
    pred = z.copy()
    holes = np.zeros(z.shape, np.uint8)
    holes[30:80, 40:100] = 1
    pred[30:80, 40:100] += rng.normal(0, 0.3, (50, 60)).astype(np.float32)
    pred[33, 44] = np.nan                                           # a pixel the fill left: unknown on both sides
    d = wetness_errors(z, pred, holes, cellsize=2.0, exponent=4, min_slope=0.01)
    assert d == wetness_errors(z, pred, holes, cellsize=2.0, exponent=np.int64(4), min_slope=0.01)     # numpy's integers too
    counts, sums, sides = wetness_raw(z, pred, holes, cellsize=2.0, exponent=4, min_slope=0.01)
    assert sorted(d) == ["bias", "cells", "mae", "max", "rmse"] and d["cells"] == 50 * 60 - 1
    known = torch.from_numpy((np.isfinite(z) & np.isfinite(pred)).astype(np.uint8)).to(dev)
    twis = [wetness_known(torch.from_numpy(s).to(dev), known, 2.0, exponent=4, min_slope=0.01)[0].cpu().numpy() for s in (z, pred)]
    cells, sd, sa, s2, mx = MO.wetness_stats(holes, twis[0], twis[1])
    assert d["cells"] == cells == counts[0] and d["max"] == float(mx) and d["max"] > 0
    assert np.array([counts[1]], np.uint32).view(np.float32)[0] == mx
    for what, got, ref in (("sum d", sums[0], sd), ("sum |d|", sums[1], sa), ("sum d^2", sums[2], s2),
                           ("bias", d["bias"], sd / cells), ("mae", d["mae"], sa / cells), ("rmse", d["rmse"], (s2 / cells) ** 0.5)):
        print("wetness_errors", what, got, ref, "rel", abs(got - ref) / abs(ref))
        assert abs(got - ref) <= 1e-12 * abs(ref), (what, got, ref)
    assert [s["exponent"] for s in sides] == [4, 4] and [s["min_slope"] for s in sides] == [0.01, 0.01]
    same = wetness_errors(z, z, holes, cellsize=2.0)
    assert same == {"cells": 50 * 60, "bias": 0.0, "mae": 0.0, "rmse": 0.0, "max": 0.0}
    none = wetness_errors(z, z, np.zeros_like(holes), cellsize=2.0)
    assert none == {"cells": 0, "bias": None, "mae": None, "rmse": None, "max": None}


def test_evaluate_raster_wetness(dev):
    """End to end on the small scene of tests/test_hip_drainage.py: the GAN, the harmonic baseline and the IDW fill, each with its
    wetness entry, equal to a direct wetness_errors call on that fill; without the option the report is what it was."""
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, wetness_errors, wetness_summary
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",))
    rep, pred = evaluate_raster(G, z, wetness=True, wetness_exponent=4, **kw)
    plain, pred0 = evaluate_raster(G, z, wetness=False, **kw)                 # the report of the code as it stood
    assert torch.equal(pred, pred0)

    def strip(r):
        return {k: (strip(v) if isinstance(v, dict) and k in ("baseline", "compare", "idw") else v) for k, v in r.items()
                if k != "wetness"}
    assert "wetness" not in plain and "wetness" not in plain["baseline"] and "wetness" not in plain["compare"]["idw"]
    assert json.dumps(strip(rep)) == json.dumps(plain) and set(rep) - set(plain) == {"wetness"}
    for d in (rep["wetness"], rep["baseline"]["wetness"], rep["compare"]["idw"]["wetness"]):
        assert sorted(d) == ["bias", "cells", "mae", "max", "rmse"] and d["cells"] > 0 and d["max"] >= d["rmse"] >= d["mae"] > 0
        assert "wetness: TWI bias" in wetness_summary(d)
    zt = torch.from_numpy(z).to(dev)
    hm, keep, _ = eval_holes(zt, None, split="test", block=160, tile=80, cellsize=c)
    assert json.dumps(rep["wetness"]) == json.dumps(wetness_errors(zt, pred, hm, cellsize=c, exponent=4))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(dev):
    from mvp_gan.src.evaluate_raster import wetness_errors
    from mvp_gan.src.flow_routing import mfd_accumulation, wetness_index
    from tg_hip import ops as O
    z = FO.rounded_pits(20, 30, 1)
    for bad in (0, 9, 1.5, 2.0, True):
        with pytest.raises(ValueError, match="exponent"):
            mfd_accumulation(z, exponent=bad)
        with pytest.raises(ValueError, match="exponent"):
            wetness_index(z, exponent=bad)
        with pytest.raises(ValueError, match="exponent"):
            wetness_errors(z, z, np.ones_like(z), cellsize=1.0, exponent=bad)
    for bad in (0, 0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="min_slope"):
            wetness_index(z, min_slope=bad)
        with pytest.raises(ValueError, match="min_slope"):
            wetness_errors(z, z, np.ones_like(z), cellsize=1.0, min_slope=bad)
    acc, info = mfd_accumulation(z, exponent=np.int64(4))           # numpy's integers and reals are accepted
    assert info["exponent"] == 4 and type(info["exponent"]) is int
    assert torch.equal(acc, mfd_accumulation(z, exponent=4)[0])
    twi = wetness_index(z, exponent=np.int32(1), min_slope=np.float32(0.01))[0]
    assert torch.equal(twi, wetness_index(z, min_slope=float(np.float32(0.01)))[0])
    for bad in (np.float64(2.0), np.bool_(True)):
        with pytest.raises(ValueError, match="exponent"):
            mfd_accumulation(z, exponent=bad)
    w = torch.from_numpy(z).to(dev)
    known = torch.ones(20, 30, dtype=torch.uint8, device=dev)
    d = torch.full((20, 30), FO.OUT, dtype=torch.uint8, device=dev)
    ws = O.mfd_ws(20, 30, dev)
    for bad in (0, 9, 1.5):
        with pytest.raises(ValueError, match="exponent"):
            O.mfd_setup(w, known, d, bad, ws)
    with pytest.raises(ValueError, match="float32"):
        O.mfd_setup(w.double(), known, d, 1, ws)
    with pytest.raises(ValueError, match="float32"):
        O.terrain_slope(w.double(), known, 1.0)
    with pytest.raises(ValueError, match="float32"):
        O.wetness(w.double(), w, known, 1.0, 1e-3)
    with pytest.raises(ValueError, match="min_slope"):
        O.wetness(w, w, known, 1.0, 0.0)
    short = ws[:ws.numel() - 1]
    with pytest.raises(ValueError, match="ws must be"):
        O.mfd_setup(w, known, d, 1, short)
    A, counts = O.mfd_setup(w, known, d, 1, ws)
    with pytest.raises(ValueError, match="ws must be"):
        O.mfd_sweep(w, 1, 1, A, counts, short)
    with pytest.raises(ValueError, match="ws must be"):
        O.mfd_finish(A, d, short)
    with pytest.raises(ValueError, match="ws must be"):
        O.wetness_compare(known, w, w, short)
    # a flat raster, all OUT: every pixel is a sink and final after one sweep
    flat = torch.full((20, 30), 1000.0, device=dev)
    A, counts = O.mfd_setup(flat, known, d, 1, ws)
    assert counts.cpu().tolist() == [0, 0, 600, 600, 0]
    O.mfd_sweep(flat, 1, 1, A, counts, ws)
    assert counts.cpu().tolist()[:4] == [0, 0, 600, 0] and (A == 1.0).all()
