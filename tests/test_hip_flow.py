"""GPU checks of the flow routing (csrc/flow.hip, mvp_gan/src/flow_routing.py) against the numpy oracle of
tests/flow_oracle.py.  Directions, the flat distance D and the accumulation are compared bit for bit, the numbers of info
exactly; nothing has a tolerance."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import depfill_oracle as DO
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


def _ref(name, z, mask=None, nodata=None, fill=True):
    """The oracle of a named scene, computed once and left unchanged."""
    key = (name, fill)
    if key not in _REF:
        r = FO.route(z, mask, nodata, fill)
        for v in r.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def _distance(dev, r, max_sweeps=4096, check_every=8):
    """slope, flat sweeps and flat directions through the ops on the oracle's surface -> (dir, D, sweeps, converged, counts)."""
    from mvp_gan.src.flow_routing import resolve_flats
    from tg_hip import ops as O
    H, W = r["w"].shape
    w = torch.from_numpy(np.array(r["w"])).to(dev)
    known = torch.from_numpy(r["known"].astype(np.uint8)).to(dev)
    ws = O.flow_ws(H, W, dev)
    d, D, c0 = O.flow_slope(w, known, ws)
    sweeps, visits, conv = resolve_flats(w, D, ws, max_sweeps, check_every)
    c1 = O.flow_flat_dir(w, D, d)
    return d.cpu().numpy(), D.cpu().numpy(), sweeps, conv, c0.cpu().tolist() + c1.cpu().tolist()


def _check(dev, name, z, mask=None, nodata=None, fill=True, **kw):
    """flow_routing against the oracle: direction, D, accumulation, every number of info; -> (dir, acc, info)."""
    from mvp_gan.src.flow_routing import flow_routing
    r = _ref(name, z, mask, nodata, fill)
    direction, acc, info = flow_routing(z, mask, nodata=nodata, cellsize=2.0, fill=fill, **kw)
    assert direction.dtype == torch.uint8 and acc.dtype == torch.int32
    assert tuple(direction.shape) == tuple(acc.shape) == z.shape
    d, a = direction.cpu().numpy(), acc.cpu().numpy()
    print(name, fill, {k: info[k] for k in ("flat_cells", "pits", "flat_sweeps", "tile_visits", "acc_rounds", "max_accumulation")})
    np.testing.assert_array_equal(d, r["dir"])
    np.testing.assert_array_equal(a, r["acc"])
    d2, D, _, conv, counts = _distance(dev, r)
    assert conv
    np.testing.assert_array_equal(D, r["D"])
    np.testing.assert_array_equal(d2, r["dir"])
    known = r["known"]
    assert counts == [int(known.sum()), r["outlets"], r["flat_cells"], r["pits"]]
    assert info["converged"] is True and info["filled"] is fill
    assert (info["known"], info["unknown"]) == (int(known.sum()), int((~known).sum()))
    assert info["outlets"] == r["outlets"] and info["flat_cells"] == r["flat_cells"] and info["pits"] == r["pits"]
    assert info["max_accumulation"] == int(r["acc"].max()) and info["max_area_m2"] == 4.0 * info["max_accumulation"]
    assert info["acc_rounds"] == r["rounds"]
    assert info["flat_sweeps"] >= 1 and (info["tile_visits"] >= 1 or not known.any())
    if fill:
        assert info["pits"] == 0
    return d, a, info


# ---- shapes ------------------------------------------------------------------------------------------------------------------
def _small():
    pit = np.array([[1003, 1002, 1004], [1001, 990, 1005], [1006, 1002.5, 1007]], np.float32)
    return {"1x1": np.full((1, 1), 1000.5, np.float32), "1x300": FO.rounded_pits(1, 300, 1), "300x1": FO.rounded_pits(300, 1, 2),
            "2x2": FO.rounded_pits(2, 2, 3, npits=1), "3x3 pit": pit}


@pytest.mark.parametrize("name", list(_small()))
@pytest.mark.parametrize("fill", (True, False))
def test_small_shapes(dev, name, fill):
    z = _small()[name]
    d, a, info = _check(dev, name, z, fill=fill)
    if name == "3x3 pit" and not fill:
        assert d[1, 1] == FO.PIT and a[1, 1] == 9 and info["pits"] == 1
    if name == "1x1":
        assert d[0, 0] == FO.OUT and a[0, 0] == 1 and info["acc_rounds"] == 0


@pytest.mark.parametrize("H", (63, 64, 65, 129))
@pytest.mark.parametrize("W", (127, 128, 130))
@pytest.mark.parametrize("fill", (True, False))
def test_tile_shapes(dev, H, W, fill):
    z = FO.rounded_pits(H, W, 100 * H + W, npits=20)
    _, _, info = _check(dev, f"rounded {H}x{W}", z, fill=fill)
    assert info["flat_cells"] > 100
    if not fill:
        assert info["pits"] > 0


def _voids(H, W, seed):
    rng = np.random.default_rng(seed)
    z = FO.rounded_pits(H, W, seed, npits=12)
    mask = (rng.random((H, W)) >= 0.017).astype(np.float32)
    z[rng.random((H, W)) < 0.017] = np.nan
    z[rng.random((H, W)) < 0.017] = -9999.0
    return z, mask


@pytest.mark.parametrize("fill", (True, False))
def test_voids_are_outlets(dev, fill):
    z, mask = _voids(67, 130, 5)
    d, a, info = _check(dev, "voids 67x130", z, mask, -9999.0, fill)
    assert 0.03 < info["unknown"] / z.size < 0.07
    assert int((d == 0).sum()) == info["unknown"] and int((a == 0).sum()) == info["unknown"]


def test_negative_heights(dev):
    z = FO.rounded_pits(65, 130, 9, npits=10, base=-120.0)
    assert (z < 0).all()
    _check(dev, "negative", z, fill=True)
    _check(dev, "negative", z, fill=False)


def test_real_heights(dev):
    z = DO.pits_scene(129, 130, 11, npits=20)                              # no rounding: almost no flats without the fill
    _, _, info = _check(dev, "real", z, fill=True)
    assert info["flat_cells"] > 0
    _check(dev, "real", z, fill=False)


# ---- flats -------------------------------------------------------------------------------------------------------------------
def test_flat_raster(dev):
    z = np.full((130, 130), 1000.25, np.float32)
    d, a, info = _check(dev, "flat", z, fill=False)
    assert info["flat_cells"] == 128 * 128 and info["outlets"] == 4 * 129 and info["pits"] == 0
    edge = np.ones(z.shape, bool)
    edge[1:-1, 1:-1] = False
    assert (d[edge] == FO.OUT).all() and int(a[edge].sum()) == z.size     # every pixel drains to the edge
    assert info["flat_sweeps"] == 8                                       # three tiles across: done by the first check
    _check(dev, "flat", z, fill=True)


def test_lake_with_a_notch_at_a_tile_corner(dev):
    z, lake = FO.lake_scene()
    for fill in (False, True):
        d, a, info = _check(dev, "lake", z, fill=fill)
        assert info["flat_cells"] == int(lake.sum()) and d[64, 64] == 1 and a[64, 64] >= int(lake.sum()) + 1


def test_spiral_flat(dev):
    from mvp_gan.src.flow_routing import flow_routing
    z, channel = FO.spiral_flat()
    r = _ref("spiral flat", z, fill=False)
    assert r["D"][channel].max() > 4096                                   # the oracle itself
    d, a, info = _check(dev, "spiral flat", z, fill=False)
    assert info["flat_sweeps"] > 8                                        # the host loop went round more than once
    # Stopped early: D is an upper bound where it is finite, PIT exactly where nothing has arrived, and direction is a forest.
    # The distance travels the channel, which re-enters every tile dozens of times, and a tile is visited once per sweep: two
    # sweeps cannot suffice, whatever the order of the visits.
    d2, D2, sweeps, conv, counts = _distance(dev, r, max_sweeps=2, check_every=1)
    assert conv is False and sweeps == 2
    und = r["D"] > 0
    fin = und & (D2 < FO.FAR)
    assert (D2[fin] >= r["D"][fin]).all() and (D2[und & ~fin] == FO.FAR).all() and (und & ~fin).any()
    np.testing.assert_array_equal(D2[~und], r["D"][~und])
    np.testing.assert_array_equal(d2 == FO.PIT, und & ~fin)
    np.testing.assert_array_equal(d2, FO.flat_dirs(r["w"], FO.slope_step(r["w"], r["known"])[0], D2, exact=False))
    assert counts[2] == int(fin.sum()) and counts[3] == int((und & ~fin).sum())
    acc, _ = FO.accumulate_kahn(d2)                                       # asserts that there is no cycle
    direction, got, info = flow_routing(z, fill=False, max_sweeps=2, check_every=1)
    assert info["converged"] is False and info["flat_sweeps"] == 2 and info["pits"] > 0
    dn, an = direction.cpu().numpy(), got.cpu().numpy()
    assert info["pits"] == int((dn == FO.PIT).sum())
    np.testing.assert_array_equal(an, FO.accumulate_kahn(dn)[0])          # the accumulation of whatever forest it left
    for m in (3, 5):                                                      # a cut-off inside a batch of check_every
        _, _, info = flow_routing(z, fill=False, max_sweeps=m, check_every=2)
        assert info["flat_sweeps"] == m and info["converged"] is False
    _check(dev, "spiral flat", z, fill=True)


# ---- accumulation ------------------------------------------------------------------------------------------------------------
def test_serpentine(dev):
    z, order = FO.serpentine()
    r = _ref("serpentine", z, fill=False)
    assert r["longest"] > 4096
    d, a, info = _check(dev, "serpentine", z, fill=False)
    assert info["acc_rounds"] >= 13 and info["pits"] == 0
    mouth = np.unravel_index(np.argmax(order), order.shape)
    assert d[mouth] == FO.OUT and a[mouth] == info["max_accumulation"] > 16000
    _check(dev, "serpentine", z, fill=True)


def test_accumulation_ops(dev):
    """The rounds in batches of every size, a stop before the end, the state they report."""
    from tg_hip import ops as O
    z, _ = FO.serpentine()
    r = _ref("serpentine", z, fill=False)
    d = torch.from_numpy(np.array(r["dir"])).to(dev)
    ws = O.flow_ws(130, 130, dev)
    state = torch.zeros(2, dtype=torch.int32, device=dev)
    for batch in (1, 5, 32):
        O.flow_accum_init(d, ws)
        k, seen = 0, []
        while k < 32:
            n = min(batch, 32 - k)
            O.flow_accum(130, 130, k, n, state, ws)
            k += n
            seen.append(state.cpu().tolist())
            if seen[-1][0] == 0:
                break
        assert seen[-1] == [0, r["rounds"]] and all(s[0] > 0 and s[1] == (i + 1) * batch for i, s in enumerate(seen[:-1]))
        acc, amax = O.flow_accum_finish(130, 130, seen[-1][1], ws)
        np.testing.assert_array_equal(acc.cpu().numpy(), r["acc"])
        assert int(amax.item()) == int(r["acc"].max())
    # after k rounds S counts the pixels fewer than 2^k steps upstream
    O.flow_accum_init(d, ws)
    O.flow_accum(130, 130, 0, 3, state, ws)
    assert state.cpu().tolist()[1] == 3
    acc, _ = O.flow_accum_finish(130, 130, 3, ws)
    nxt = FO.receivers(r["dir"])
    S = (r["dir"].ravel() != 0).astype(np.int64)
    for _ in range(3):
        live = nxt >= 0
        S2 = S.copy()
        np.add.at(S2, nxt[live], S[live])
        n2 = np.full_like(nxt, -1)
        n2[live] = nxt[nxt[live]]
        S, nxt = S2, n2
    np.testing.assert_array_equal(acc.cpu().numpy().ravel(), S)


def test_reproducible_and_check_every(dev):
    from mvp_gan.src.flow_routing import flow_routing
    z, mask = _voids(129, 130, 6)
    sp, _ = FO.spiral_flat()
    se, _ = FO.serpentine()
    for zz, mm in ((z, mask), (sp, None), (se, None)):
        outs = [flow_routing(zz, mm, nodata=-9999.0, check_every=n) for n in (8, 8, 1, 64)]
        assert all(i["converged"] and i["pits"] == 0 for _, _, i in outs)
        for d, a, i in outs[1:]:
            assert torch.equal(d, outs[0][0]) and torch.equal(a, outs[0][1])
            assert {k: v for k, v in i.items() if k not in ("flat_sweeps", "tile_visits")} == \
                {k: v for k, v in outs[0][2].items() if k not in ("flat_sweeps", "tile_visits")}
        assert outs[3][2]["flat_sweeps"] % 64 == 0 and outs[0][2]["flat_sweeps"] % 8 == 0


def test_empty(dev):
    from mvp_gan.src.flow_routing import flow_routing
    for fill in (True, False):
        d, a, info = flow_routing(np.full((70, 65), np.nan, np.float32), fill=fill)
        assert not d.any() and not a.any() and info["converged"] is True
        assert (info["known"], info["unknown"], info["outlets"], info["flat_cells"], info["pits"], info["max_accumulation"],
                info["max_area_m2"], info["acc_rounds"]) == (0, 70 * 65, 0, 0, 0, 0, 0.0, 0)


# ---- front ends --------------------------------------------------------------------------------------------------------------
def test_inputs_numpy_and_tensor(dev):
    from mvp_gan.src.flow_routing import flow_routing, streams, to_esri
    z, mask = _voids(67, 130, 5)
    r = _ref("voids 67x130", z, mask, -9999.0, True)
    for zz, mm in ((z, mask), (torch.from_numpy(z).to(dev), torch.from_numpy(mask).to(dev)), (z, mask != 0),
                   (torch.from_numpy(z).to(dev), torch.from_numpy(mask != 0).to(dev))):
        d, a, info = flow_routing(zz, mm, nodata=-9999.0)
        np.testing.assert_array_equal(d.cpu().numpy(), r["dir"])
        np.testing.assert_array_equal(a.cpu().numpy(), r["acc"])
    e = to_esri(d)
    assert e.is_cuda and e.dtype == torch.uint8
    np.testing.assert_array_equal(e.cpu().numpy(), to_esri(r["dir"]))
    s = streams(a, 50)
    assert s.is_cuda and s.dtype == torch.uint8 and 0 < int(s.sum()) < int(r["known"].sum())
    np.testing.assert_array_equal(s.cpu().numpy(), (r["acc"] >= 50).astype(np.uint8))
    d, a, _ = flow_routing(z, mask, nodata=float("nan"))                    # a NaN nodata is ignored: -9999 is a height then
    r2 = FO.route(z, mask, None, True)
    np.testing.assert_array_equal(d.cpu().numpy(), r2["dir"])
    np.testing.assert_array_equal(a.cpu().numpy(), r2["acc"])
    with pytest.raises(ValueError, match="pass a numpy array or a HIP tensor"):
        flow_routing(torch.from_numpy(z))


def test_cli(dev, tmp_path):
    from mvp_gan.src.flow_routing import to_esri
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    z, mask = _voids(67, 130, 5)
    z[np.isnan(z)] = -9999.0
    dem, mpath, dout, aout, sout = (str(tmp_path / n) for n in ("dem.asc", "mask.asc", "dir.asc", "acc.asc", "streams.asc"))
    _write_asc(dem, z, 0.5, -9999)
    _write_asc(mpath, mask, 0.5)
    zr, _ = read_asc(dem)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    r = FO.route(zr, mask, -9999.0, True)
    p = subprocess.run([sys.executable, "-m", "mvp_gan.src.flow_routing", "--dem", dem, "--dir-out", dout, "--acc-out", aout,
                        "--mask", mpath, "--streams-out", sout, "--min-cells", "40", "--esri"], cwd=cwd, capture_output=True,
                       text=True, timeout=600)                              # one start of the CLI; --no-fill is the parser test's
    assert p.returncode == 0, p.stderr
    amax = int(r["acc"].max())
    assert f"{int(r['known'].sum())} cells, {r['outlets']} outlets, {r['flat_cells']} flat cells, {r['pits']} pits" in p.stdout
    assert f"largest contributing area {amax} cells = {0.25 * amax:.6g} m2" in p.stdout
    got, hdr = read_asc(dout)
    np.testing.assert_array_equal(got, to_esri(r["dir"]).astype(np.float32))
    assert dict(hdr)["cellsize"] == "0.5" and "NODATA_value" not in dict(hdr)
    got, _ = read_asc(aout)
    np.testing.assert_array_equal(got, r["acc"].astype(np.float32))
    got, _ = read_asc(sout)
    np.testing.assert_array_equal(got, (r["acc"] >= 40).astype(np.float32))
