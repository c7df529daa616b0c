"""GPU checks of the depression fill (csrc/depfill.hip, mvp_gan/src/fill_depressions.py, the sink statistics of
mvp_gan/src/evaluate_raster.py) against the priority-flood of tests/depfill_oracle.py.  Rasters are compared bit for bit (uint32
views, NaN at the same places); counts, the largest depth and the number of depressions exactly; the fp64 depth sum within
(2 n + 4) 2^-53 S for n raised pixels of sum S: the terms are exact and non-negative, so any order of summation is within
(n - 1) 2^-53 S of the true sum, and the oracle's is correctly rounded."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depfill_oracle as DO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """Bitwise, with NaN at the same places (whatever its payload)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.where(np.isnan(want), 0, _bits(got)), np.where(np.isnan(want), 0, _bits(want)))


def _ref(name, z, mask=None, nodata=None, conn=8):
    """The oracle of a named scene, computed once: (known, W, out, depth, flags, stats)."""
    key = (name, conn)
    if key not in _REF:
        known = DO.known_map(z, mask, nodata)
        w = DO.priority_flood(z, known, conn)
        out, depth, flags = DO.finish(z, w, known)
        _REF[key] = (known, w, out, depth, flags, DO.stats(z, w, known))
        for v in _REF[key][:5]:
            v.setflags(write=False)
    return _REF[key]


def _sum_ok(got, st):
    return abs(got - st["depth_sum"]) <= (2 * st["raised"] + 4) * 2.0 ** -53 * st["depth_sum"]


def _check(name, z, mask=None, nodata=None, conn=8, **kw):
    """fill_depressions against the oracle: raster, depth, every number of info; -> (out numpy, info)."""
    from mvp_gan.src.fill_depressions import fill_depressions
    known, w, want, wdepth, flags, st = _ref(name, z, mask, nodata, conn)
    out, depth, info = fill_depressions(z, mask, nodata=nodata, connectivity=conn, want_depth=True, cellsize=2.0, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == z.shape
    o = out.cpu().numpy()
    print(name, conn, {k: info[k] for k in ("raised", "sweeps", "tile_visits", "depth_sum_m")}, st["depth_sum"])
    _same(o, want)
    _same(depth.cpu().numpy(), wdepth)
    keep = known & (flags == 0)
    np.testing.assert_array_equal(_bits(o)[keep], _bits(z)[keep])           # un-raised known pixels are z's own bits
    assert info["converged"] is True and info["unreached"] == 0 and info["connectivity"] == conn
    assert (info["known"], info["unknown"]) == (int(known.sum()), int((~known).sum()))
    assert info["outlets"] == int(DO.outlets(known, conn).sum())
    assert info["raised"] == st["raised"] and info["max_depth_m"] == st["max_depth"]
    assert info["depressions"] == DO.depressions(flags)
    assert _sum_ok(info["depth_sum_m"], st), (info["depth_sum_m"], st)
    assert info["volume_m3"] == 4.0 * info["depth_sum_m"]
    assert info["sweeps"] >= 1 and info["tile_visits"] >= 1
    return o, info


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _small():
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    return {"1x1": np.full((1, 1), 1000.5, np.float32), "1x300": DO.pits_scene(1, 300, 1), "300x1": DO.pits_scene(300, 1, 2),
            "2x2": DO.pits_scene(2, 2, 3, npits=1), "3x3 pit": pit}


@pytest.mark.parametrize("name", list(_small()))
@pytest.mark.parametrize("conn", (8, 4))
def test_small_shapes(dev, name, conn):
    z = _small()[name]
    out, info = _check(name, z, conn=conn)
    if name == "3x3 pit":
        assert out[1, 1] == np.float32(1001) and info["raised"] == 1 and info["depressions"] == 1
    else:
        assert info["raised"] == 0                                           # every pixel is on the edge: all are outlets


@pytest.mark.parametrize("H", (63, 64, 65, 129))
@pytest.mark.parametrize("W", (127, 128, 130))
def test_tile_shapes(dev, H, W):
    z = DO.pits_scene(H, W, 100 * H + W, npits=20)
    _, info = _check(f"pits {H}x{W}", z, conn=8 if (H + W) % 2 else 4)
    assert info["raised"] > 0


def _voids(H, W, seed):
    rng = np.random.default_rng(seed)
    z = DO.pits_scene(H, W, seed, npits=12)
    mask = (rng.random((H, W)) >= 0.017).astype(np.float32)
    z[rng.random((H, W)) < 0.017] = np.nan
    z[rng.random((H, W)) < 0.017] = -9999.0
    return z, mask


@pytest.mark.parametrize("conn", (8, 4))
def test_voids_are_outlets(dev, conn):
    z, mask = _voids(67, 130, 5)
    out, info = _check("voids 67x130", z, mask, -9999.0, conn)
    assert 0.03 < info["unknown"] / z.size < 0.07 and np.isnan(out).sum() == info["unknown"]


def test_negative_heights(dev):
    z = DO.pits_scene(65, 130, 9, npits=10, base=-120.0)
    assert (z < 0).all() and not (np.signbit(z) & (z == 0)).any()
    _check("negative", z)


# ---- tile seams --------------------------------------------------------------------------------------------------------------
def _ground(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return (1005.0 + 0.02 * x + 0.01 * y + rng.normal(0, 0.05, (H, W))).astype(np.float32)


def _seams():
    s = {}
    z = DO.bowl(_ground(130, 130, 1), 63.5, 63.5, 9, 992.0, 0.7)
    z[63, 63] = 991.0                                                        # the lowest point: the corner of four tiles
    s["corner of four tiles"] = z
    z = _ground(67, 200, 2)
    z[29:34, 8:183] = 1010.0                                                 # a dyke around
    z[30:33, 10:181] = 990.0                                                 # a trough through three tiles
    z[31, 181:200] = 995.0                                                   # its only spill: a notch in the far tile, to the edge
    s["three tiles, far spill"] = z
    z = DO.bowl(_ground(130, 130, 3), 64, 70, 22, 992.0, 0.3)
    y, x = np.mgrid[0:130, 0:130]
    r = np.hypot(y - 64, x - 62)
    z[(r > 4.5) & (r <= 6.5)] = 996.5                                        # the inner rim
    z[r <= 4.5] = (989.0 + 0.2 * r[r <= 4.5]).astype(np.float32)             # the pit in the pit
    s["nested"] = z
    for d, name in ((1, "void next to the low point"), (2, "void one pixel further")):
        z = DO.bowl(_ground(130, 130, 4), 64, 64, 10, 990.0, 0.8)
        z[64, 64 + d] = np.nan
        s[name] = z
    return s


@pytest.mark.parametrize("name", list(_seams()))
def test_tile_seams(dev, name):
    z = _seams()[name]
    out, info = _check(name, z)
    if name == "corner of four tiles":
        assert out[63, 63] > z[63, 63] and out[63, 63] == out[64, 64] == out[63, 64] == out[64, 63]
    if name == "three tiles, far spill":
        assert (out[30:33, 10:181] == np.float32(995.0)).all()
    if name == "nested":
        assert out[64, 62] == out[64, 70] > np.float32(996.5)                # one lake over both
    if name == "void next to the low point":
        y, x = np.mgrid[0:130, 0:130]
        inside = np.hypot(y - 64, x - 64) <= 10
        inside[64, 65] = False
        np.testing.assert_array_equal(_bits(out)[inside], _bits(z)[inside])  # the void is its outlet: nothing fills
    if name == "void one pixel further":
        assert out[64, 64] == z[64, 65] > z[64, 64]                          # up to the outlet's height


@pytest.mark.parametrize("conn", (8, 4))
def test_diagonal_gap(dev, conn):
    z = np.full((130, 130), 980.0, np.float32)
    z[50:81, 50:81] = DO.gap_scene(31, 10, 20)                               # the wall crosses the tile seams at 63/64
    out, info = _check("diagonal gap", z, conn=conn)
    if conn == 8:
        assert info["raised"] == 0
    else:
        assert info["raised"] == 81 and (out[61:70, 61:70] == np.float32(1020.0)).all() and info["depressions"] == 1


# ---- the spiral --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", (8, 4))
def test_spiral(dev, conn):
    from mvp_gan.src.fill_depressions import fill_depressions
    z, channel = DO.spiral_scene()
    level = np.float32(1040.0 if conn == 8 else 1050.0)
    known, w, want, _, flags, st = _ref("spiral", z, conn=conn)
    assert (want[channel] == level).all() and st["raised"] == int(channel.sum()) > 12000        # the oracle itself
    out, info = _check("spiral", z, conn=conn)
    assert info["sweeps"] > 8                                                # the host loop went round more than once
    # Stopped early: an upper bound everywhere, NaN exactly where nothing has arrived.  The level travels the channel, which
    # re-enters every tile many times, and a tile is visited once per sweep: two sweeps cannot suffice, whatever the order of
    # the visits, so some pixel is still above the answer and the last sweep lowered something.  (The wall is known and finite,
    # so a finite bound, 1100 m, does reach every pixel of these 3 x 3 tiles within two sweeps: unreached is 0 or more here;
    # a state with unreached pixels is checked in test_stats_and_finish_ops.)
    part, pinfo = fill_depressions(z, connectivity=conn, max_sweeps=2, check_every=1)
    p = part.cpu().numpy()
    print("spiral, 2 sweeps:", pinfo)
    assert pinfo["converged"] is False and pinfo["sweeps"] == 2 and pinfo["unreached"] >= 0
    assert int(np.isnan(p).sum()) == pinfo["unreached"]                      # no unknown pixel in this scene
    fin = ~np.isnan(p)
    assert (p[fin] >= want[fin]).all() and ((p[fin] > want[fin]).any() or pinfo["unreached"] > 0)
    for m in (3, 5):                                                         # a cut-off inside a batch of check_every
        _, pinfo = fill_depressions(z, connectivity=conn, max_sweeps=m, check_every=2)
        assert pinfo["sweeps"] == m and pinfo["converged"] is False


# ---- properties --------------------------------------------------------------------------------------------------------------
def test_flat_and_empty(dev):
    from mvp_gan.src.fill_depressions import fill_depressions
    z = np.full((130, 200), 1000.25, np.float32)
    out, info = fill_depressions(z)
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(z))
    assert info["raised"] == 0 and info["depressions"] == 0 and info["converged"] and info["sweeps"] == 8   # the first check
    assert info["depth_sum_m"] == 0.0 and info["max_depth_m"] == 0.0 and info["outlets"] == 2 * 130 + 2 * 198
    out, info = fill_depressions(np.full((70, 65), np.nan, np.float32))
    assert np.isnan(out.cpu().numpy()).all() and info["converged"]
    assert (info["known"], info["unknown"], info["outlets"], info["raised"], info["depressions"]) == (0, 70 * 65, 0, 0, 0)


def test_reproducible_and_check_every(dev):
    from mvp_gan.src.fill_depressions import fill_depressions
    z, mask = _voids(129, 130, 6)
    a, ia = fill_depressions(z, mask, nodata=-9999.0)
    b, ib = fill_depressions(z, mask, nodata=-9999.0)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and ia["depth_sum_m"] == ib["depth_sum_m"]
    sp, _ = DO.spiral_scene()
    for zz, mm in ((z, mask), (sp, None)):
        outs = [fill_depressions(zz, mm, nodata=-9999.0, check_every=n) for n in (1, 8, 64)]
        assert all(i["converged"] for _, i in outs)
        for o, _ in outs[1:]:
            assert torch.equal(o.view(torch.int32), outs[0][0].view(torch.int32))
        assert outs[2][1]["sweeps"] % 64 == 0 and outs[1][1]["sweeps"] % 8 == 0


# ---- statistics and finish -------------------------------------------------------------------------------------------------
def test_stats_and_finish_ops(dev):
    from mvp_gan.src.fill_depressions import relax
    from tg_hip import ops as O
    z, mask = _voids(129, 130, 6)
    known, w, want, wdepth, wflags, st = _ref("voids 129x130", z, mask, -9999.0)
    zt = torch.from_numpy(np.nan_to_num(z, nan=123.0)).to(dev)               # z at unknown pixels is never read as a height
    kt = torch.from_numpy(known.astype(np.uint8)).to(dev)
    wt, outlets, sweeps, visits, conv = relax(zt, kt)
    assert conv and outlets == int(DO.outlets(known).sum())
    _same(wt.cpu().numpy(), w)                                               # the state itself: NaN at unknown pixels
    counts, sums = O.depfill_stats(zt, wt, kt)
    c, s = counts.cpu().tolist(), sums.cpu().tolist()
    assert c == [st["raised"], 0, st["counted"]] and s[1] == st["max_depth"] and _sum_ok(s[0], st)
    c2, s2 = O.depfill_stats(zt, wt, kt)
    assert torch.equal(c2, counts) and torch.equal(s2.view(torch.int64), sums.view(torch.int64))
    sel = np.zeros(z.shape, np.uint8)
    sel[20:90, 33:101] = 7
    rs = DO.stats(z, w, known, sel)
    assert 0 < rs["raised"] < st["raised"]
    counts, sums = O.depfill_stats(zt, wt, kt, torch.from_numpy(sel).to(dev))
    c, s = counts.cpu().tolist(), sums.cpu().tolist()
    assert c == [rs["raised"], 0, rs["counted"]] and s[1] == rs["max_depth"] and _sum_ok(s[0], rs)
    out, depth, flags = O.depfill_finish(zt, wt, kt, want_depth=True, want_flags=True)
    _same(out.cpu().numpy(), want)
    _same(depth.cpu().numpy(), wdepth)
    np.testing.assert_array_equal(flags.cpu().numpy(), wflags)
    o2, d2, f2 = O.depfill_finish(zt, wt, kt)
    assert d2 is None and f2 is None and torch.equal(o2.view(torch.int32), out.view(torch.int32))
    # the state after init alone: outlets at z, the rest +inf, counted as unreached
    ws = O.depfill_ws(129, 130, dev)
    w0 = O.depfill_init(zt, kt, 8, ws)
    _same(w0.cpu().numpy(), DO.relax_start(z, known))
    counts, sums = O.depfill_stats(zt, w0, kt)
    n_in = int(known.sum()) - outlets
    assert counts.cpu().tolist() == [n_in, n_in, int(known.sum())] and sums.cpu().tolist() == [0.0, 0.0]
    out, depth, flags = O.depfill_finish(zt, w0, kt, want_depth=True, want_flags=True)
    assert int(torch.isnan(out).sum()) == n_in + int((~known).sum()) and int(flags.sum()) == n_in


# ---- front ends --------------------------------------------------------------------------------------------------------------
def test_inputs_numpy_and_tensor(dev):
    from mvp_gan.src.fill_depressions import fill_depressions
    z, mask = _voids(67, 130, 5)
    want = _ref("voids 67x130", z, mask, -9999.0)[2]
    for zz, mm in ((z, mask), (torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev)), (z, mask != 0),
                   (torch.from_numpy(z).to(dev), torch.from_numpy(mask != 0).to(dev))):
        out, info = fill_depressions(zz, mm, nodata=-9999.0)
        _same(out.cpu().numpy(), want)
    out, _ = fill_depressions(z, mask, nodata=math.nan)                      # a NaN nodata is ignored: -9999 is a height then
    known = DO.known_map(z, mask)
    _same(out.cpu().numpy(), DO.finish(z, DO.priority_flood(z, known), known)[0])
    with pytest.raises(ValueError, match="pass a numpy array or a HIP tensor"):
        fill_depressions(torch.from_numpy(z))


def test_cli(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    z, mask = _voids(67, 130, 5)
    z[np.isnan(z)] = -9999.0
    dem, mpath, out, dout = (str(tmp_path / n) for n in ("dem.asc", "mask.asc", "filled.asc", "depth.asc"))
    _write_asc(dem, z, 0.5, -9999)
    _write_asc(mpath, mask, 0.5)
    zr, _ = read_asc(dem)
    known = DO.known_map(zr, mask, -9999.0)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    for conn in (8, 4):
        w = DO.priority_flood(zr, known, conn)
        want, wdepth, flags = DO.finish(zr, w, known)
        r = subprocess.run([sys.executable, "-m", "mvp_gan.src.fill_depressions", "--dem", dem, "--out", out, "--mask", mpath,
                            "--connectivity", str(conn), "--depth-out", dout], cwd=cwd, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr
        assert f"{int(flags.sum())} of {int(known.sum())} cells raised in {DO.depressions(flags)} depressions" in r.stdout
        got, hdr = read_asc(out)
        nd = np.float32(-9999.0)
        np.testing.assert_array_equal(_bits(got), _bits(np.where(np.isnan(want), nd, want)))
        got, _ = read_asc(dout)
        np.testing.assert_array_equal(_bits(got), _bits(np.where(np.isnan(wdepth), nd, wdepth)))
        assert dict(hdr)["cellsize"] == "0.5"


def _sink_scene():
    from tests.test_hip_terrain_eval import _terrain
    H = W = 256
    z = _terrain(H, W, 2.0, 21)
    holes = np.zeros((H, W), np.uint8)
    holes[40:100, 50:120] = 1
    holes[150:230, 30:90] = 1
    holes[120:200, 140:240] = 1
    pred = z.copy()
    for y, x, d in ((60, 64, 3.0), (190, 60, 2.0), (128, 192, 4.5)):          # one of them on a tile corner
        pred[y - 2:y + 3, x - 2:x + 3] -= np.float32(d)
    return z, pred, holes


def _sink_oracle(z, pred, holes, c):
    known = DO.known_map(z) & DO.known_map(pred)
    side = []
    for s in (z, pred):
        w = DO.priority_flood(s, known)
        st = DO.stats(s, w, known, holes)
        with np.errstate(invalid="ignore"):
            st["depressions"] = DO.depressions(known & (w > s) & (holes != 0))
        side.append(st)
    return side


def test_sink_errors(dev):
    from mvp_gan.src.evaluate_raster import sink_errors
    z, pred, holes = _sink_scene()
    c = 2.0
    t, p = _sink_oracle(z, pred, holes, c)
    s = sink_errors(z, pred, holes, cellsize=c)
    print(s)
    assert p["raised"] > t["raised"] > 0 and p["depth_sum"] > t["depth_sum"]
    for got, st in ((s["truth"], t), (s["pred"], p)):
        assert got["cells"] == st["raised"] and got["max_depth_m"] == st["max_depth"] and got["converged"] is True
        assert got["depressions"] == st["depressions"]
        assert abs(got["volume_m3"] - c * c * st["depth_sum"]) <= c * c * (2 * st["raised"] + 5) * 2.0 ** -53 * st["depth_sum"]
    assert s["excess_cells"] == p["raised"] - t["raised"]
    assert s["excess_volume_m3"] == s["pred"]["volume_m3"] - s["truth"]["volume_m3"]
    tol = c * c * 2.0 ** -53 * ((2 * p["raised"] + 6) * p["depth_sum"] + (2 * t["raised"] + 6) * t["depth_sum"])
    assert abs(s["excess_volume_m3"] - c * c * (p["depth_sum"] - t["depth_sum"])) <= tol
    same = sink_errors(z, z.copy(), torch.from_numpy(holes).to(dev), cellsize=c)
    assert same["excess_cells"] == 0 and same["excess_volume_m3"] == 0.0 and same["truth"] == same["pred"] == s["truth"]
    nanp = pred.copy()
    nanp[10:20, 10:20] = np.nan                                              # a fill that left pixels out: unknown for both
    s2 = sink_errors(z, nanp, holes, cellsize=c)
    assert s2["pred"]["converged"] and s2["excess_cells"] > 0


def test_evaluate_raster_sinks(dev):
    """End to end on the small scene of tests/test_hip_idw.py: the GAN, the harmonic baseline and the IDW fill, each with its
    sinks entry, equal to a direct sink_errors call on that fill; without sinks the report is what it was."""
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, sink_errors, sinks_summary
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",))
    rep, pred = evaluate_raster(G, z, sinks=True, **kw)
    plain, pred0 = evaluate_raster(G, z, **kw)
    off, _ = evaluate_raster(G, z, sinks=False, **kw)
    assert torch.equal(pred, pred0)

    def strip(r):
        return {k: (strip(v) if isinstance(v, dict) and k in ("baseline", "compare", "idw") else v) for k, v in r.items()
                if k != "sinks"}
    assert "sinks" not in plain and "sinks" not in plain["baseline"] and "sinks" not in plain["compare"]["idw"]
    assert json.dumps(off) == json.dumps(plain) and json.dumps(strip(rep)) == json.dumps(plain)
    assert set(rep) - set(plain) == {"sinks"}
    zt = torch.from_numpy(z).to(dev)
    hm, keep, _ = eval_holes(zt, None, split="test", block=160, tile=80, cellsize=c)
    assert json.dumps(rep["sinks"]) == json.dumps(sink_errors(zt, pred, hm, cellsize=c))
    bpred, _ = fill_voids(zt, keep, method="laplace")
    assert json.dumps(rep["baseline"]["sinks"]) == json.dumps(sink_errors(zt, bpred, hm, cellsize=c))
    ipred, _ = interpolate_voids(zt, keep, method="idw", cellsize=c)
    assert json.dumps(rep["compare"]["idw"]["sinks"]) == json.dumps(sink_errors(zt, ipred, hm, cellsize=c))
    sides = [rep["sinks"], rep["baseline"]["sinks"], rep["compare"]["idw"]["sinks"]]
    assert all(s["truth"] == sides[0]["truth"] for s in sides)                # the same truth on the same holes
    for s in sides:
        assert s["truth"]["converged"] and s["pred"]["converged"] and "excess" in sinks_summary(s)
        assert s["excess_cells"] == s["pred"]["cells"] - s["truth"]["cells"]
