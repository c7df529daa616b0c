"""GPU checks of the watersheds, the flow length and the drainage comparison (csrc/drainage.hip, mvp_gan/src/flow_routing.py
watersheds, mvp_gan/src/evaluate_raster.py drainage_errors) against the numpy oracle of
tests/drainage_oracle.py.  Basins, step counts and the bits of the lengths are compared bit for bit, the counters and every
number derived from them exactly; nothing has a tolerance."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import drainage_oracle as DR
from tests import flow_oracle as FO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REF = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _route(name, z, fill=True, mask=None):
    """The oracle's routing of a named scene, computed once and left unchanged."""
    key = (name, fill)
    if key not in _REF:
        r = FO.route(z, mask, None, fill)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _ops_paths(dev, code, pour=None, cellsize=1.0, batch=8):
    """The doubling through the ops -> (basin, nc, nd, length as numpy, counts, rounds, pour counts, the states seen)."""
    from tg_hip import ops as O
    H, W = code.shape
    d = torch.from_numpy(np.array(code)).to(dev)
    pr = None if pour is None else torch.from_numpy(np.ascontiguousarray(pour, np.uint8)).to(dev)
    ws = O.flow_basin_ws(H, W, dev)
    pc = O.flow_basin_init(d, pr, ws)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    k, seen = 0, []
    while k < 32:
        n = min(batch, 32 - k)
        O.flow_basin(H, W, k, n, state, ws)
        k += n
        seen.append(state.cpu().tolist())
        if seen[-1][0] == 0:
            break
    rounds = seen[-1][1]
    basin, nc, nd, ln, counts = O.flow_basin_finish(H, W, rounds, ws, cellsize, want_steps=True)
    return (basin.cpu().numpy(), nc.cpu().numpy(), nd.cpu().numpy(), ln.cpu().numpy(), counts.cpu().tolist(), rounds,
            pc.cpu().tolist(), seen)


def _check(dev, code, pour=None, cellsize=1.0, **kw):
    """watersheds and the ops against the oracle: basin, nc, nd, the bits of length_m, every number of info -> (oracle, info)."""
    from mvp_gan.src.flow_routing import watersheds
    w = DR.watersheds(code, pour, cellsize)
    basin, ln, info = watersheds(code, pour, cellsize=cellsize, **kw)
    assert basin.dtype == torch.int32 and ln.dtype == torch.float32 and basin.is_cuda and ln.is_cuda
    assert tuple(basin.shape) == tuple(ln.shape) == code.shape
    np.testing.assert_array_equal(basin.cpu().numpy(), w["T"])
    np.testing.assert_array_equal(_bits(ln.cpu().numpy()), _bits(w["length"]))
    assert info == {"basins": w["basins"], "rounds": w["rounds"], "longest_steps": w["longest"], "max_length_m": w["max_length"],
                    "pour_points": w["used"], "pour_ignored": w["ignored"]}
    b, nc, nd, l2, counts, rounds, pc, _ = _ops_paths(dev, code, pour, cellsize)
    np.testing.assert_array_equal(b, w["T"])
    np.testing.assert_array_equal(nc, w["nc"])
    np.testing.assert_array_equal(nd, w["nd"])
    np.testing.assert_array_equal(_bits(l2), _bits(w["length"]))
    assert counts == [w["basins"], w["longest"], int(_bits(np.float32(w["max_length"])).ravel()[0])] and rounds == w["rounds"]
    assert pc == [w["used"], w["ignored"]]
    return w, info


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _small():
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    return {"1x1": np.full((1, 1), 1000.5, np.float32), "1x300": FO.rounded_pits(1, 300, 1), "300x1": FO.rounded_pits(300, 1, 2),
            "2x2": FO.rounded_pits(2, 2, 3, npits=1), "3x3 pit": pit}


@pytest.mark.parametrize("name", list(_small()))
def test_small_shapes(dev, name):
    z = _small()[name]
    r = _route(name, z, fill=False)
    w, info = _check(dev, r["dir"])
    if name == "3x3 pit":
        assert info["basins"] == 1 and (w["T"] == 4).all() and info["longest_steps"] == 1 and r["dir"][1, 1] == FO.PIT
        assert info["max_length_m"] == float(np.float32(DR.SQRT2))
    if name == "1x1":
        assert info == {"basins": 1, "rounds": 0, "longest_steps": 0, "max_length_m": 0.0, "pour_points": 0, "pour_ignored": 0}


@pytest.mark.parametrize("H", (63, 64, 65, 129))
@pytest.mark.parametrize("W", (127, 128, 130))
def test_tile_shapes(dev, H, W):
    z = FO.rounded_pits(H, W, 100 * H + W, npits=20)
    r = _route(f"rounded {H}x{W}", z, fill=True)
    w, info = _check(dev, r["dir"], cellsize=2.0)
    assert info["basins"] > 10 and info["rounds"] >= 3 and (w["nd"] > 0).any() and (w["nc"] > 0).any()


def _voids():
    """67x130 with 5 % voids, half by the mask and half NaN -> (z, mask)."""
    rng = np.random.default_rng(5)
    z = FO.rounded_pits(67, 130, 5, npits=12)
    mask = (rng.random(z.shape) >= 0.025).astype(np.float32)
    z[rng.random(z.shape) < 0.025] = np.nan
    return z, mask


def _voids_route():
    z, mask = _voids()
    return _route("voids 67x130", z, True, mask)


def test_voids(dev):
    r = _voids_route()
    assert 0.03 < (~r["known"]).mean() < 0.07
    w, info = _check(dev, r["dir"])
    assert (w["T"][~r["known"]] == -1).all() and (w["length"][~r["known"]] == 0).all()


def test_serpentine(dev):
    """8130 steps, 13 rounds: a record torn between two iterates or a wrong final plane would show here."""
    z, order = FO.serpentine()
    r = _route("serpentine", z, fill=False)
    w, info = _check(dev, r["dir"])
    assert info["longest_steps"] == 8130 and info["rounds"] == 13 and info["rounds"] % 2 == 1
    on = order >= 0
    steps = (w["nc"] + w["nd"])[on][np.argsort(order[on])]
    assert steps[0] == 8129 and steps[-1] == 0 and (np.diff(steps) <= 0).all()      # the place along the channel, corners cut
    _check(dev, _route("serpentine", z, fill=True)["dir"])


def test_spiral_flat(dev):
    z, channel = FO.spiral_flat()
    r = _route("spiral flat", z, fill=False)
    w, info = _check(dev, r["dir"], cellsize=0.5)
    assert info["longest_steps"] > 4096 and info["rounds"] >= 13


def test_empty(dev):
    from mvp_gan.src.flow_routing import watersheds
    code = np.zeros((70, 65), np.uint8)
    w, info = _check(dev, code)
    assert info == {"basins": 0, "rounds": 0, "longest_steps": 0, "max_length_m": 0.0, "pour_points": 0, "pour_ignored": 0}
    basin, ln, _ = watersheds(code, compact=True)
    assert not basin.any() and not ln.any()


# ---- the rounds --------------------------------------------------------------------------------------------------------------
def test_basin_ops(dev):
    """The rounds in batches of every size, the state they report, and the records after three rounds."""
    from tg_hip import ops as O
    z, _ = FO.serpentine()
    r = _route("serpentine", z, fill=False)
    w = DR.watersheds(r["dir"])
    for batch in (1, 5, 32):
        b, nc, nd, ln, counts, rounds, _, seen = _ops_paths(dev, r["dir"], batch=batch)
        assert seen[-1] == [0, w["rounds"]] and all(s[0] > 0 and s[1] == (i + 1) * batch for i, s in enumerate(seen[:-1]))
        np.testing.assert_array_equal(b, w["T"])
        np.testing.assert_array_equal(nc, w["nc"])
        np.testing.assert_array_equal(nd, w["nd"])
    d = torch.from_numpy(np.array(r["dir"])).to(dev)
    ws = O.flow_basin_ws(130, 130, dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    for k in (0, 3, 4):
        O.flow_basin_init(d, None, ws)
        if k:
            O.flow_basin(130, 130, 0, k, state, ws)
            assert state.cpu().tolist()[1] == k
        basin, nc, nd, _, _ = O.flow_basin_finish(130, 130, k, ws, want_steps=True, want_length=False)
        last, c, dg, _ = DR.paths_doubling(r["dir"], max_rounds=k)
        np.testing.assert_array_equal(basin.cpu().numpy(), last)
        np.testing.assert_array_equal(nc.cpu().numpy(), c)
        np.testing.assert_array_equal(nd.cpu().numpy(), dg)


def test_reproducible_and_check_every(dev):
    from mvp_gan.src.flow_routing import watersheds
    se, _ = FO.serpentine()
    for code in (_voids_route()["dir"], _route("serpentine", se, fill=False)["dir"]):
        outs = [watersheds(code, cellsize=2.0, check_every=n) for n in (8, 8, 1, 64)]
        for b, ln, i in outs[1:]:
            assert torch.equal(b, outs[0][0]) and torch.equal(ln.view(torch.int32), outs[0][1].view(torch.int32))
            assert i == outs[0][2]


# ---- pour points, labels, front ends -----------------------------------------------------------------------------------------
def test_pour_points(dev):
    z, order = FO.serpentine()
    r = _route("serpentine", z, fill=False)
    pour = (order == 4000).astype(np.uint8)
    w, info = _check(dev, r["dir"], pour)
    pp = int(np.flatnonzero(pour.ravel())[0])
    mouth = int(np.flatnonzero(order.ravel() == order.max())[0])
    on = order >= 0
    assert (w["T"][on & (order <= 4000)] == pp).all() and (w["T"][on & (order > 4000)] == mouth).all()
    assert info["pour_points"] == 1 and info["pour_ignored"] == 0
    # many pour points, some on unknown pixels, other dtypes
    rv = _voids_route()
    rng = np.random.default_rng(9)
    pour = (rng.random(rv["dir"].shape) < 0.04)
    pour[~rv["known"]] |= rng.random(int((~rv["known"]).sum())) < 0.3
    w, info = _check(dev, rv["dir"], pour.astype(np.float32) * 3.5)
    assert info["pour_points"] > 100 and info["pour_ignored"] > 20
    _check(dev, rv["dir"], pour)
    w0 = DR.watersheds(rv["dir"])
    assert info["basins"] > w0["basins"]


def test_compact_labels(dev):
    from mvp_gan.src.flow_routing import watersheds
    code = _voids_route()["dir"]
    w = DR.watersheds(code)
    basin, _, info = watersheds(code, compact=True)
    got = basin.cpu().numpy()
    assert basin.dtype == torch.int32
    np.testing.assert_array_equal(got, DR.compact(w["T"]))
    u, inv = np.unique(w["T"][w["T"] >= 0], return_inverse=True)
    assert got.max() == len(u) == info["basins"] and (got[w["T"] < 0] == 0).all()
    np.testing.assert_array_equal(got[w["T"] >= 0], inv.ravel() + 1)


def test_inputs_numpy_and_tensor(dev):
    from mvp_gan.src.flow_routing import flow_routing, watersheds
    zv, mask = _voids()
    r = _voids_route()
    w = DR.watersheds(r["dir"], None, 2.0)
    pour = np.zeros(zv.shape, bool)
    pour[20, 30] = pour[0, 0] = True
    wp = DR.watersheds(r["dir"], pour, 2.0)
    direction, _, _ = flow_routing(zv, mask)
    for d in (np.array(r["dir"]), torch.from_numpy(np.array(r["dir"])).to(dev), direction):
        basin, ln, _ = watersheds(d, cellsize=2.0)
        np.testing.assert_array_equal(basin.cpu().numpy(), w["T"])
        np.testing.assert_array_equal(_bits(ln.cpu().numpy()), _bits(w["length"]))
        for pr in (pour, torch.from_numpy(pour).to(dev), torch.from_numpy(pour.astype(np.int32)).to(dev)):
            basin, ln, info = watersheds(d, pr, cellsize=2.0)
            np.testing.assert_array_equal(basin.cpu().numpy(), wp["T"])
            assert info["pour_points"] == wp["used"]
    with pytest.raises(ValueError, match="pass a numpy array or a HIP tensor"):
        watersheds(torch.from_numpy(np.array(r["dir"])))
    bad = np.array(r["dir"])
    bad[5, 5] = 254
    with pytest.raises(ValueError, match="254"):
        watersheds(bad)


def test_cli(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    z, _ = _voids()
    z[np.isnan(z)] = -9999.0
    dem, pr, dout, aout, bout, lout = (str(tmp_path / n) for n in ("dem.asc", "pour.asc", "d.asc", "a.asc", "b.asc", "l.asc"))
    _write_asc(dem, z, 0.5, -9999)
    pour = np.zeros(z.shape, np.float32)
    pour[20, 30] = pour[40, 100] = 1
    _write_asc(pr, pour, 0.5)
    zr, _ = read_asc(dem)
    r = FO.route(zr, None, -9999.0, True)
    w = DR.watersheds(r["dir"], pour, 0.5)
    p = subprocess.run([sys.executable, "-m", "mvp_gan.src.flow_routing", "--dem", dem, "--dir-out", dout, "--acc-out", aout,
                        "--basins-out", bout, "--pour", pr, "--compact", "--length-out", lout],
                       cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    assert f"{w['basins']} basins, longest path {w['longest']} steps = {w['max_length']:.9g} m, {w['rounds']} rounds" in p.stdout
    got, hdr = read_asc(bout)
    np.testing.assert_array_equal(got, DR.compact(w["T"]).astype(np.float32))
    assert "NODATA_value" not in dict(hdr) and dict(hdr)["cellsize"] == "0.5"
    got, _ = read_asc(lout)
    np.testing.assert_array_equal(_bits(got), _bits(w["length"]))               # full float32 precision
    assert len(np.unique(w["length"])) > 50


# ---- flow_compare ------------------------------------------------------------------------------------------------------------
def _compare(dev, planes, stream_cells, tol2):
    from tg_hip import ops as O
    names = ("sel", "dt", "dp", "bt", "bp", "at", "ap", "d2t", "d2p")
    t = [torch.from_numpy(np.ascontiguousarray(planes[k], np.uint8 if i < 3 else np.int32)).to(dev) for i, k in enumerate(names)]
    got = dict(zip(O.FLOW_COMPARE_NAMES, O.flow_compare(*t, stream_cells, tol2).cpu().tolist()))
    want = DR.compare(*[planes[k] for k in names], stream_cells, tol2)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    return got


def _planes(H, W):
    z = np.zeros((H, W), np.int32)
    return {"sel": np.ones((H, W), np.uint8), "dt": np.ones((H, W), np.uint8), "dp": np.ones((H, W), np.uint8), "bt": z.copy(),
            "bp": z.copy(), "at": z + 1, "ap": z + 1, "d2t": z.copy(), "d2p": z.copy()}


def test_flow_compare_every_counter(dev):
    H, W = 5, 70                                                           # more than one wave, not a multiple of one
    base = _compare(dev, _planes(H, W), 4, 2)
    n = H * W
    assert [base[k] for k in DR.NAMES[:5]] == [n] * 5 and all(base[k] == 0 for k in DR.NAMES[5:])
    rng = np.random.default_rng(3)
    p = _planes(H, W)
    p["sel"][0, :10] = 0
    p["dt"][1, :7] = 0
    p["dp"][2, :5] = 0
    assert _compare(dev, p, 4, 2)["cells"] == n - 22
    p = _planes(H, W)
    p["dt"][:] = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 255], np.uint8), (H, W))
    p["dp"][:] = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, 9, 255], np.uint8), (H, W))
    c = _compare(dev, p, 4, 2)
    assert 0 < c["dir_equal"] < c["dir_within_45"] < c["dir_routed"] < c["cells"] == n
    for a, b, near in ((1, 8, 1), (8, 1, 1), (1, 2, 1), (3, 3, 1), (1, 3, 0), (2, 6, 0), (9, 9, 0), (255, 255, 0), (8, 9, 0)):
        p = _planes(1, 1)
        p["dt"][:], p["dp"][:] = a, b
        c = _compare(dev, p, 4, 2)
        assert (c["dir_within_45"], c["dir_equal"], c["dir_routed"]) == (near, int(a == b), int(a <= 8 and b <= 8))
    p = _planes(H, W)
    p["bt"][:] = rng.integers(0, n, (H, W))
    p["bp"][:] = np.where(rng.random((H, W)) < 0.3, p["bt"], rng.integers(0, n, (H, W)))
    c = _compare(dev, p, 4, 2)
    assert 0 < c["same_outlet"] < n and c["outlet_d2_max"] > 0 and c["outlet_d2_sum"] > c["outlet_d2_max"]
    p = _planes(H, W)
    p["at"][:] = rng.integers(1, 2 ** 22, (H, W))
    p["ap"][:] = 1 << rng.integers(0, 31, (H, W))
    p["at"][0, :4] = (1, 2 ** 31 - 1, 2 ** 30, 2 ** 30 - 1)
    p["ap"][0, :4] = (2 ** 31 - 1, 1, 2 ** 30 - 1, 2 ** 30)
    c = _compare(dev, p, 1 << 20, 2)
    assert c["area_octave_sum"] > 30 + 30 + 1 + 1 and 0 < c["streams_both"] < min(c["streams_truth"], c["streams_pred"])
    p = _planes(H, W)
    p["at"][:] = rng.integers(1, 9, (H, W))
    p["ap"][:] = rng.integers(1, 9, (H, W))
    p["d2t"][:] = rng.integers(0, 7, (H, W))
    p["d2p"][:] = rng.integers(0, 50000, (H, W))
    for tol2 in (0, 2, 6):
        c = _compare(dev, p, 5, tol2)
        assert c["pred_far"] == c["truth_far"] == 0 and c["pred_d2_max"] == 6 and c["truth_d2_max"] > 40000
        assert 0 < c["pred_matched"] <= c["streams_pred"] and c["truth_d2_sum"] > c["pred_d2_sum"] > 0
    assert c["pred_matched"] == c["streams_pred"]
    # TG_EDT_FAR: counted, and kept out of the sums and maxima
    p["d2t"][rng.random((H, W)) < 0.3] = DR.EDT_FAR
    c = _compare(dev, p, 5, 6)
    assert 0 < c["pred_far"] < c["streams_pred"] and c["pred_matched"] + c["pred_far"] == c["streams_pred"] and c["pred_d2_max"] == 6
    p["d2p"][:] = DR.EDT_FAR
    c = _compare(dev, p, 5, 6)
    assert c["truth_far"] == c["streams_truth"] > 0 and (c["truth_matched"], c["truth_d2_sum"], c["truth_d2_max"]) == (0, 0, 0)


def test_flow_compare_sums_above_32_bits(dev):
    H = W = 300
    p = _planes(H, W)
    p["bp"][:] = H * W - 1                                                  # every terminal pair at opposite corners
    p["at"][:] = p["ap"][:] = 7
    p["d2t"][:] = 2 * 32766 ** 2                                           # the largest distance of an admitted raster
    p["d2p"][:] = 2 ** 31 - 2
    c = _compare(dev, p, 7, 9)
    assert c["outlet_d2_sum"] == H * W * 2 * 299 ** 2 > 2 ** 32 and c["outlet_d2_max"] == 2 * 299 ** 2
    assert c["pred_d2_sum"] == H * W * 2 * 32766 ** 2 > 2 ** 47 and c["truth_d2_sum"] == H * W * (2 ** 31 - 2)
    assert c["pred_far"] == c["truth_far"] == 0 and c["truth_d2_max"] == 2 ** 31 - 2


# ---- drainage_errors ---------------------------------------------------------------------------------------------------------
def _scene_ref():
    if "scene" not in _REF:
        z, pred, holes = DR.scene()
        c, rep, sides = DR.drainage(z, pred, holes, DR.CELLSIZE, DR.STREAM_CELLS, DR.TOL_PX ** 2, DR.TOL_PX * DR.CELLSIZE)
        _REF["scene"] = (z, pred, holes, c, rep, sides)
    return _REF["scene"]


def test_drainage_errors_against_the_oracle(dev):
    from mvp_gan.src.evaluate_raster import drainage_errors, drainage_raw, drainage_summary
    z, pred, holes, c, rep, sides = _scene_ref()
    counts, got_sides, tol_m, tol2 = drainage_raw(z, pred, holes, cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS)
    assert (tol_m, tol2) == (6.0, 9)
    assert dict(zip(DR.NAMES, counts)) == c
    d = drainage_errors(z, pred, holes, cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS)
    print(json.dumps(d))
    assert d == rep                                                         # every derived number with ==
    assert d["truth"]["rounds"] == d["pred"]["rounds"] == 8 and d["cells"] == 10200
    assert d == drainage_errors(torch.from_numpy(z).to(dev), torch.from_numpy(pred).to(dev), torch.from_numpy(holes).to(dev),
                                cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS, stream_tol_m=6.0)
    assert "precision 0.809" in drainage_summary(d)
    # another threshold and tolerance
    c2, rep2, _ = DR.drainage(z, pred, holes, DR.CELLSIZE, 400, 5, 4.5)       # floor(2.25^2)
    d2 = drainage_errors(z, pred, holes, cellsize=DR.CELLSIZE, stream_cells=400, stream_tol_m=4.5)
    assert d2 == rep2 and d2["streams"]["pred_cells"] < d["streams"]["pred_cells"]


def test_drainage_errors_identity_and_nan(dev):
    from mvp_gan.src.evaluate_raster import drainage_errors
    z, pred, holes, c, rep, sides = _scene_ref()
    d = drainage_errors(z, z.copy(), holes, cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS)
    assert d["direction"]["equal"] == d["direction"]["within_45"] == d["outlet"]["same"] == 1.0
    assert d["outlet"]["shift_rms_m"] == d["outlet"]["shift_max_m"] == 0.0 and d["area"]["octave_mae"] == 0.0
    s = d["streams"]
    assert s["precision"] == s["recall"] == 1.0 and s["truth_cells"] == s["pred_cells"] == s["both_cells"] == c["streams_truth"]
    assert s["pred_to_truth_rms_m"] == s["pred_to_truth_max_m"] == s["truth_to_pred_rms_m"] == s["truth_to_pred_max_m"] == 0.0
    assert d["truth"] == d["pred"] == rep["truth"] and d["cells"] == 10200
    # a fill that left pixels out: unknown on both sides
    nanp = pred.copy()
    nanp[40:50, 50:62] = np.nan
    d = drainage_errors(z, nanp, holes, cellsize=DR.CELLSIZE, stream_cells=DR.STREAM_CELLS)
    assert d["cells"] == 10200 - 120
    assert d == DR.drainage(z, nanp, holes, DR.CELLSIZE, DR.STREAM_CELLS, 9, 6.0)[1]


def test_evaluate_raster_drainage(dev):
    """End to end on the small scene of tests/test_hip_depfill.py: the GAN, the harmonic baseline and the IDW fill, each with its
    drainage entry, equal to a direct drainage_errors call on that fill; without the option the report is what it was."""
    from mvp_gan.src.evaluate_raster import drainage_errors, drainage_summary, eval_holes, evaluate_raster
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.interpolate import interpolate_voids
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",))
    dk = dict(stream_cells=200, stream_tol_m=5.0)
    rep, pred = evaluate_raster(G, z, drainage=True, **dk, **kw)
    before = pred.clone()
    plain, pred0 = evaluate_raster(G, z, **kw)                                # the parent's call
    off, _ = evaluate_raster(G, z, drainage=False, **dk, **kw)
    assert torch.equal(pred, pred0)

    def strip(r):
        return {k: (strip(v) if isinstance(v, dict) and k in ("baseline", "compare", "idw") else v) for k, v in r.items()
                if k != "drainage"}
    assert "drainage" not in plain and "drainage" not in plain["baseline"] and "drainage" not in plain["compare"]["idw"]
    assert json.dumps(off) == json.dumps(plain) and json.dumps(strip(rep)) == json.dumps(plain)
    assert set(rep) - set(plain) == {"drainage"}
    zt = torch.from_numpy(z).to(dev)
    hm, keep, _ = eval_holes(zt, None, split="test", block=160, tile=80, cellsize=c)
    assert json.dumps(rep["drainage"]) == json.dumps(drainage_errors(zt, pred, hm, cellsize=c, **dk))
    bpred, _ = fill_voids(zt, keep, method="laplace")
    assert json.dumps(rep["baseline"]["drainage"]) == json.dumps(drainage_errors(zt, bpred, hm, cellsize=c, **dk))
    ipred, _ = interpolate_voids(zt, keep, method="idw", cellsize=c)
    assert json.dumps(rep["compare"]["idw"]["drainage"]) == json.dumps(drainage_errors(zt, ipred, hm, cellsize=c, **dk))
    assert torch.equal(pred, before)                                           # pred is unchanged
    sides = [rep["drainage"], rep["baseline"]["drainage"], rep["compare"]["idw"]["drainage"]]
    assert all(s["truth"] == sides[0]["truth"] and s["cells"] == sides[0]["cells"] > 0 for s in sides)
    for s in sides:
        assert s["stream_cells"] == 200 and s["stream_tol_m"] == 5.0 and s["truth"]["converged"] and s["pred"]["converged"]
        assert "drainage:" in drainage_summary(s) and s["streams"]["truth_cells"] == sides[0]["streams"]["truth_cells"]
