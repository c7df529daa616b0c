"""GPU checks of the natural-neighbour (discrete Sibson) void fill (csrc/natural.hip, mvp_gan/src/natural.py,
mvp_gan/src/evaluate_raster.py) against the numpy oracle in tests/natural_oracle.py.

The kernel sums in row-major order of q, the oracle's order, so every scene is compared bit for bit.  Two further checks do not
lean on that choice:
  - exact scenes: heights that are multiples of 2^-8 m near 1000 m carry 19 significant bits, a window has at most 63^2 < 2^12
    contributors, so every fp64 sum is exact in any order and the comparison is bit for bit whatever order a kernel takes;
  - general scenes: |out - oracle| <= 1 ulp of fp32 at max(|lo|, |hi|): two fp64 sums of fewer than 2^12 terms differ by less
    than 2^-40 relative, and the one rounding to fp32 moves that by at most one ulp; the largest error is printed.
support and counts are integers and always exact."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import idw_oracle as IO
from tests import natural_oracle as NO
from tests.test_hip_idw import _dirty_raster, _heights, _one, _random

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TH, TW = 4, 64                                                # natural.hip's tile; checked against ops.NATURAL_TILE below
RADII = (1, 2, 5, 32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    from tg_hip import ops as O
    lib.load()
    assert O.NATURAL_TILE == (TH, TW)
    return torch.device("cuda:0")


def _t(dev, a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def _exact(z):
    """Multiples of 2^-8 m: every fp64 sum of fewer than 2^12 of them is exact."""
    q = (np.round(z.astype(np.float64) * 256.0) / 256.0).astype(np.float32)
    assert (q.astype(np.float64) * 256.0 == np.round(q.astype(np.float64) * 256.0)).all() and np.abs(q).max() < 2048
    return q


# ---- scenes: name -> (z, known, exact) ---------------------------------------------------------------------------------------
def _checker_and_block():
    """A checkerboard (depth 1) on the left, a 40x60 void on the right of the same raster: the tiles of the left columns see
    only shallow maxima within their reach, those next to the void see deep ones."""
    H, W = 70, 200
    y, x = np.mgrid[0:H, 0:W]
    known = np.ones((H, W), np.uint8)
    known[:, :100] = ((y + x) & 1)[:, :100]
    known[15:55, 125:185] = 0
    return known


def _tile_scenes():
    out = {}
    for H in (TH - 1, TH, TH + 1, 2 * TH + 1):
        for W in (TW - 1, TW, TW + 1, 2 * TW + 1):
            blk = _random(H, W, 0.3, 100 * H + W)
            blk[max(TH - 2, 0):TH + 3, TW - 5:TW + 6] = 0            # a void block across the corner (TH, TW) of the first tile
            blk[0, 0] = 1
            out[f"{H}x{W} block"] = (_heights(H, W, H + W), blk, False)
            out[f"{H}x{W} corner seed"] = (_exact(_heights(H, W, H + W + 1)), _one(H, W, H - 1, W - 1), True)
    return out


def _scenes():
    out = {"1x1 known": (_heights(1, 1, 1), np.ones((1, 1), np.uint8)), "1x1 void": (_heights(1, 1, 2), np.zeros((1, 1), np.uint8)),
           "1x300": (_heights(1, 300, 3), _random(1, 300, 0.01, 1)), "300x1": (_heights(300, 1, 4), _random(300, 1, 0.01, 2)),
           "130x67 p=0.2": (_heights(130, 67, 1), _random(130, 67, 0.2, 21)),
           "65x130 p=0.02": (_heights(65, 130, 2), _random(65, 130, 0.02, 22)),
           "70x90 one seed": (_heights(70, 90, 4), _one(70, 90, 33, 41)),
           "all known": (_heights(9, 129, 5), np.ones((9, 129), np.uint8)),
           "none known": (_heights(9, 129, 6), np.zeros((9, 129), np.uint8)),
           "checkerboard and block": (_heights(70, 200, 7), _checker_and_block())}
    full = {}
    for name, (z, known) in out.items():
        full[name] = (z, known, False)
        full[name + " exact"] = (_exact(z), known, True)
    full.update(_tile_scenes())
    return full


SCENES = _scenes()
_ORACLE = {}


def _oracle(name, radius, lim2=0):
    """Computed once per (scene, radius, limit) and shared; the arrays are read-only."""
    key = (name, radius, lim2)
    if key not in _ORACLE:
        z, known, _ = SCENES[name]
        res = NO.natural(z, known, radius, lim2)
        for a in res:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _ORACLE[key] = res
    return _ORACLE[key]


def _run(dev, z, known, radius, lim2=0, want_support=True):
    """The chain of natural_neighbour_voids on given planes -> (out, support or None, counts, nn, d2) as numpy."""
    from tg_hip import ops as O
    zt, kt = _t(dev, z), _t(dev, known, np.uint8)
    d2, idx = O.edt_nearest(kt, 0)
    nn, _ = O.gather_fill(zt, kt, idx)
    out, counts, sup = O.natural_fill(nn, d2, kt, radius, lim2, want_support=want_support)
    assert out.dtype == torch.float32 and counts.dtype == torch.int64 and (sup is None) == (not want_support)
    if sup is not None:
        assert sup.dtype == torch.int32
    return out.cpu().numpy(), None if sup is None else sup.cpu().numpy(), counts.cpu().tolist(), nn.cpu().numpy(), d2.cpu().numpy()


def _check(dev, name, radius, lim2=0):
    z, known, exact = SCENES[name]
    want, wsup, wc, lo, hi = _oracle(name, radius, lim2)
    got, sup, counts, nn, _ = _run(dev, z, known, radius, lim2)
    kn = known != 0
    np.testing.assert_array_equal(sup, wsup)
    assert counts == wc and sum(counts) == int((~kn).sum())
    np.testing.assert_array_equal(_bits(got[kn]), _bits(z[kn]))                    # known pixels bit for bit
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    f = ~np.isnan(lo)
    assert int(f.sum()) == wc[0]
    if f.any():
        ulp = np.spacing(np.maximum(np.abs(lo[f]), np.abs(hi[f])).astype(np.float32))
        err = np.abs(got[f].astype(np.float64) - want[f].astype(np.float64))
        print(f"{name}, radius {radius}, lim2 {lim2}: max |out - oracle| / ulp = {(err / ulp).max():.3g} over {int(f.sum())} px, "
              f"largest support {int(sup.max())}")
        assert (err <= ulp).all()
        assert (got[f] >= lo[f]).all() and (got[f] <= hi[f]).all()
    np.testing.assert_array_equal(_bits(got), _bits(want))        # row-major sums on both sides (and any order on exact scenes)
    if radius == 1:
        np.testing.assert_array_equal(_bits(got), _bits(nn))      # the nearest fill, as gather_fill wrote it
    return got, sup, counts


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", [n for n in SCENES if " block" not in n and "corner seed" not in n])
def test_fill_is_the_oracle(dev, name, radius):
    got, sup, counts = _check(dev, name, radius)
    z, known, _ = SCENES[name]
    if name.startswith("none known"):
        assert np.isnan(got).all() and counts == [0, known.size] and sup.min() >= 1
    if name.startswith("all known"):
        assert counts == [0, 0] and not sup.any()
    if name.startswith("1x1 void"):
        assert np.isnan(got).all() and counts == [0, 1] and sup.tolist() == [[1]]
    if name.startswith("checkerboard and block") and radius == 32:
        assert (sup[:, :90][known[:, :90] == 0] == 1).all() and sup.max() > 100       # depth 1 beside a deep void


@pytest.mark.parametrize("H", [TH - 1, TH, TH + 1, 2 * TH + 1])
@pytest.mark.parametrize("W", [TW - 1, TW, TW + 1, 2 * TW + 1])
def test_tile_edges(dev, H, W):
    """Sides one short of, equal to, one past a tile and past two tiles: a void block across a tile corner, and one seed in the
    far corner so that the halos cross tile and raster edges at every radius."""
    for kind in ("block", "corner seed"):
        for radius in RADII:
            _check(dev, f"{H}x{W} {kind}", radius)


def test_one_seed_radius_8_support_193(dev):
    """A void deeper than the radius fills without a fallback: the nearest fill averaged over the open disc."""
    for name in ("70x90 one seed", "70x90 one seed exact"):
        got, sup, counts = _check(dev, name, 8)
        z, known, _ = SCENES[name]
        assert sup.max() == 193 and sup[10, 10] == 193 and counts == [70 * 90 - 1, 0]
        assert (got[known == 0] == z[33, 41]).all()


def test_tile_maxima(dev):
    """The pre-pass on its own: the largest c of every 4 x 64 tile."""
    from tg_hip import ops as O
    for name in ("65x130 p=0.02", "checkerboard and block", "70x90 one seed", "none known", "all known"):
        z, known, _ = SCENES[name]
        H, W = known.shape
        d2 = IO.nearest(known)[0]
        for radius in (1, 5, 32):
            c = np.minimum(d2.astype(np.int64), radius * radius)
            pad = np.zeros((-(-H // TH) * TH, -(-W // TW) * TW), np.int64)
            pad[:H, :W] = c
            want = pad.reshape(pad.shape[0] // TH, TH, pad.shape[1] // TW, TW).max(axis=(1, 3))
            got = O.natural_tile_maxima(_t(dev, d2), radius)
            assert got.dtype == torch.uint16
            np.testing.assert_array_equal(got.cpu().numpy().astype(np.int64), want)


@pytest.mark.parametrize("radius", [2, 5, 32])
def test_constant_field_comes_back_constant(dev, radius):
    for known in (_random(130, 67, 0.03, 31), _one(70, 90, 33, 41), _checker_and_block()):
        z = np.full(known.shape, 1234.5678, np.float32)
        got, sup, counts, _, _ = _run(dev, z, known, radius)
        assert (got == z).all() and counts == [int((known == 0).sum()), 0] and sup.max() > 1


@pytest.mark.parametrize("radius", [5, 32])
def test_second_call_and_support_switch(dev, radius):
    for name in ("65x130 p=0.02", "checkerboard and block", "9x129 block"):
        z, known, _ = SCENES[name]
        a, sup, ca, _, _ = _run(dev, z, known, radius)
        b, sup2, cb, _, _ = _run(dev, z, known, radius)
        c, none, cc, _, _ = _run(dev, z, known, radius, want_support=False)
        assert none is None and ca == cb == cc
        np.testing.assert_array_equal(_bits(a), _bits(b))
        np.testing.assert_array_equal(_bits(a), _bits(c))
        np.testing.assert_array_equal(sup, sup2)


@pytest.mark.parametrize("lim2", [1, 2, 25])
def test_limit_masks_the_output_only(dev, lim2):
    for name in ("65x130 p=0.02", "65x130 p=0.02 exact", "70x90 one seed"):
        z, known, _ = SCENES[name]
        for radius in (2, 5, 32):
            free, fsup, fc, _, d2 = _run(dev, z, known, radius)
            got, sup, counts = _check(dev, name, radius, lim2)
            far = (known == 0) & (d2 > lim2)
            assert far.any() and counts == [fc[0] - int(far.sum()), int(far.sum())]
            np.testing.assert_array_equal(np.isnan(got), far)
            np.testing.assert_array_equal(_bits(got[~far]), _bits(free[~far]))
            np.testing.assert_array_equal(sup, fsup)


def test_ops_rejections(dev):
    from tg_hip import lib as L
    from tg_hip import ops as O
    nn = torch.zeros(8, 9, device=dev)
    d2 = torch.zeros(8, 9, dtype=torch.int32, device=dev)
    kn = torch.ones(8, 9, dtype=torch.uint8, device=dev)
    for radius in (0, 33, 2.5, True):
        with pytest.raises(L.TgError, match="radius"):
            O.natural_fill(nn, d2, kn, radius)
    with pytest.raises(L.TgError):
        O.natural_fill(nn, d2.float(), kn)
    with pytest.raises(L.TgError):
        O.natural_fill(nn, d2, kn[:, :8].contiguous())
    with pytest.raises(L.TgError, match="lim2"):
        O.natural_fill(nn, d2, kn, lim2=2 ** 31)
    out, counts, sup = O.natural_fill(nn, d2, kn)
    assert torch.equal(out, nn) and counts.tolist() == [0, 0] and sup is None


# ---- the public API and the CLI ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,md,radius", [(1.0, None, 32), (0.25, 1.3, 5), (2.5, 12.0, 8)])
def test_natural_neighbour_voids(dev, c, md, radius):
    from mvp_gan.src.natural import natural_neighbour_voids
    H, W = 100, 150
    z, mask = _dirty_raster(H, W, 32)
    K = (mask != 0) & np.isfinite(z) & (z != np.float32(-9999.0))
    lim2 = IO.ray_px2(md, c) if md else 0
    if md:
        assert c * math.sqrt(lim2) <= md < c * math.sqrt(lim2 + 1)
    want, wsup, wc, _, _ = NO.natural(z, K, radius, lim2)
    info_want = {"unknown": int((~K).sum()), "filled": wc[0], "unfilled": wc[1], "method": "natural", "radius": radius,
                 "max_distance": md, "lim2": lim2 or None, "max_support": int(wsup.max())}
    assert (wc[1] > 0) == bool(md) and wsup.max() > 20
    out, info = natural_neighbour_voids(z, mask, nodata=-9999.0, cellsize=c, radius=radius, max_distance=md)
    np.testing.assert_array_equal(_bits(out.cpu().numpy()), _bits(want))
    assert info == info_want
    out2, sup, info2 = natural_neighbour_voids(_t(dev, z), _t(dev, mask), nodata=-9999.0, cellsize=c, radius=radius,
                                               max_distance=md, support=True)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and info2 == info_want
    np.testing.assert_array_equal(sup.cpu().numpy(), wsup)
    assert sup.dtype == torch.int32 and out.is_cuda
    out, info = natural_neighbour_voids(np.full((9, 11), np.nan, np.float32), radius=radius)
    assert np.isnan(out.cpu().numpy()).all() and (info["unknown"], info["filled"], info["unfilled"]) == (99, 0, 99)


def test_default_radius_is_32(dev):
    from mvp_gan.src.natural import natural_neighbour_voids
    z, known, _ = SCENES["70x90 one seed"]
    out, sup, info = natural_neighbour_voids(np.where(known != 0, z, np.float32(np.nan)), support=True)
    np.testing.assert_array_equal(sup.cpu().numpy(), _oracle("70x90 one seed", 32)[1])
    assert info["radius"] == 32 and info["max_support"] == int(_oracle("70x90 one seed", 32)[1].max()) > 193


def test_cli_round_trip(dev, tmp_path):
    from mvp_gan.src.asc import read_asc
    from tests.test_hip_terrain_eval import _write_asc
    H, W, c = 100, 150, 0.5
    z, mask = _dirty_raster(H, W, 33)
    z[np.isnan(z)] = -9999.0
    dem, mpath, out, spath = (str(tmp_path / n) for n in ("dem.asc", "mask.asc", "filled.asc", "support.asc"))
    _write_asc(dem, z, c, -9999)
    _write_asc(mpath, mask, c)
    zr, _ = read_asc(dem)                                   # the heights as the text round trip leaves them
    K = (mask != 0) & (zr != np.float32(-9999.0))
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda args: subprocess.run([sys.executable, "-m", "mvp_gan.src.natural", "--dem", dem, "--out", out] + args,
                                      cwd=cwd, capture_output=True, text=True, timeout=600)
    r = run(["--mask", mpath, "--radius", "8", "--support-out", spath])
    assert r.returncode == 0, r.stderr
    assert f"{int((~K).sum())} void pixels" in r.stdout and "radius 8" in r.stdout
    got, hdr = read_asc(out)
    want, wsup, wc, _, _ = NO.natural(zr, K, 8)
    np.testing.assert_array_equal(_bits(got), _bits(want))  # 9 digits: float32 reads back bit for bit
    assert dict(hdr)["cellsize"] == str(c) and not (got == -9999.0).any() and wc[1] == 0
    sup, _ = read_asc(spath)
    np.testing.assert_array_equal(sup.astype(np.int32), wsup)
    r = run(["--mask", mpath, "--radius", "3", "--max-distance", "2"])
    assert r.returncode == 0, r.stderr
    got, _ = read_asc(out)
    lim2 = IO.ray_px2(2.0, c)
    assert lim2 == 16
    want, _, wc, _, _ = NO.natural(zr, K, 3, lim2)
    assert np.isnan(want).any() and f"{wc[1]} left unfilled" in r.stdout
    np.testing.assert_array_equal(_bits(got), _bits(np.where(np.isnan(want), np.float32(-9999.0), want)))


def test_evaluate_raster_natural(dev):
    """End to end on the scene of test_hip_idw's test_evaluate_raster_compare: the natural-neighbour row on the same holes, keep
    mask and depth classes; without the keyword the report is what it was."""
    from mvp_gan.src.evaluate_raster import evaluate_raster, summary
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",),
              depth_edges_m=(2, 5, 10))
    rep, pred = evaluate_raster(G, z, natural=True, **kw)
    plain, pred0 = evaluate_raster(G, z, **kw)
    assert torch.equal(pred, pred0) and "natural" not in plain
    assert json.dumps({k: v for k, v in rep.items() if k != "natural"}) == json.dumps(plain)
    r = rep["natural"]
    key = lambda d: [(k["lo_m"], k["hi_m"], k["pixels"]) for k in d["by_depth"]["classes"]]
    assert r["method"] == "natural" and r["fill"]["method"] == "natural" and r["fill"]["radius"] == 32
    assert r["fill"]["unfilled"] == 0 and r["fill"]["unknown"] == r["fill"]["filled"] >= rep["pixels"]["holes"]
    assert r["pixels"] == dict(rep["baseline"]["pixels"]) and r["pixels"]["scored"] == rep["pixels"]["scored"] > 0
    assert r["holes"]["count"] == rep["holes"]["count"] == rep["baseline"]["holes"]["count"]
    assert key(r) == key(rep) == key(rep["baseline"]) and r["by_depth"]["cap_m"] == 10.0
    assert math.isfinite(r["height"]["rmse"]) and "by depth" in summary(r)
    assert r["fill"]["max_support"] > 1
    print(f"height RMSE: natural {r['height']['rmse']:.4f} m, idw {rep['compare']['idw']['height']['rmse']:.4f} m, "
          f"harmonic {rep['baseline']['height']['rmse']:.4f} m")
