"""GPU checks of the seam correction (csrc/seam.hip, mvp_gan/src/seam_correct.py) against the fp64 numpy oracle in
tests/seam_oracle.py and a closed form.

Bound on every oracle case: max |u - u*| <= 2e-5 x range(D over its fixed pixels) + 4 x 2^-23 x max|z|.  The first term is
the bound tests/test_hip_fill_voids.py asserts for the solver, applied to the delta raster it is given here; the second covers
the fp32 roundings of the ring target (one at <= 3 max|z|) and of the final add (one at <= max|z|), about 1.3 x 2^-23 max|z|,
with a factor 3; the maximum principle keeps ring errors from growing inward.

max_delta is compared within 2 ulp (fp32, at the oracle's value) of the oracle's.  The terrain of these tests lies within one
binade (850 .. 970 m, and so do the fills), which is what makes so tight a comparison meaningful: 2 z_q - z_q2 is then a
multiple of the inputs' ulp below 1024 and the fma is exact, e - g is exact (Sterbenz), and what is left are the roundings of
at most three additions and one division at the magnitude of the delta itself.

Also: info counts equal to the oracle's, known pixels bit for bit (a -0.0 among them), unfilled holes NaN, bitwise determinism,
convergence; inpaint_raster(seam=...), its order with the fallback, evaluate_raster(seam=...) and the CLIs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO
from tests import seam_oracle as SO
from tests import vfill_oracle as VO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVER_BOUND = 2e-5                 # x range of the delta raster over its fixed pixels
ROUND_BOUND = 4 * 2.0 ** -23        # x max |z|
INFO_KEYS = {"ring", "interior", "unfilled", "order", "max_delta", "cycles", "change", "tol", "converged"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def G(dev):
    from mvp_gan.src.models import PConvUNet
    torch.manual_seed(11)
    return PConvUNet().to(dev)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _fill(z, seed, known=None):
    """A fill of every pixel: the terrain plus an offset, a smooth error and noise; rubbish at the known pixels (never read)."""
    H, W = z.shape
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    g = np.where(np.isfinite(z) & (z > 0), z, np.float32(900.0)).astype(np.float64)
    g = (g + 1.7 + 0.9 * np.sin(x / 11.0) * np.cos(y / 13.0) + rng.normal(0, 0.2, (H, W))).astype(np.float32)
    if known is not None:
        junk = np.array([np.nan, 1e30, -np.inf, 0.0], np.float32)[rng.integers(0, 4, (H, W))]
        g = np.where(known, junk, g)
    return g


def _ulp(v):
    return float(np.spacing(np.float32(abs(v))))


def _check(z, filled, mask=None, nodata=None, order=1):
    """correct_seams against the oracle; -> (out, info, worst error / bound)."""
    from mvp_gan.src.seam_correct import correct_seams
    out, info = correct_seams(z, filled, mask, nodata=nodata, order=order)
    o = out.cpu().numpy()
    ref, r = SO.correct(z, filled, mask, nodata, order)
    k = r["known"]
    assert set(info) == INFO_KEYS and info["order"] == order
    assert (info["ring"], info["interior"], info["unfilled"]) == (r["ring"], r["interior"], r["unfilled"]), (info, r["ring"])
    assert info["converged"], info
    assert np.array_equal(_bits(o[k]), _bits(np.asarray(z)[k]))             # known pixels bit for bit
    hole_f = ~k & np.isfinite(filled)
    assert np.isnan(o[~k & ~hole_f]).all() and np.isfinite(o[hole_f]).all()
    md, mr = info["max_delta"], r["max_delta"]
    print(f"max_delta {md!r} oracle {mr!r}: {abs(md - mr) / _ulp(mr) if mr else 0.0:.2f} ulp")
    assert abs(md - mr) <= 2 * _ulp(mr) if mr else md == 0.0, (md, mr)
    ratio = 0.0
    if hole_f.any():
        D = r["D"]
        fixed = D[~np.isnan(D)]
        zmax = float(np.abs(np.asarray(z, np.float64)[k]).max()) if k.any() else 0.0      # max |z| over the known pixels
        bound = SOLVER_BOUND * (float(fixed.max() - fixed.min()) if fixed.size else 0.0) + ROUND_BOUND * zmax
        err = float(np.abs(o.astype(np.float64) - ref)[hole_f].max())
        ratio = err / bound if bound else 0.0               # nothing known: the fill comes back bit for bit, err == bound == 0
        print(f"{z.shape} order {order}: max error {err:.3g} m, bound {bound:.3g} m, ratio {ratio:.3f}, info {info}")
        assert err <= bound, (err, bound, info)
    out2, info2 = correct_seams(z, filled, mask, nodata=nodata, order=order)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and info2 == info
    return o, info, ratio


def _discs(H, W, seed, n, rmax):
    rng = np.random.default_rng(seed)
    u = np.zeros((H, W), bool)
    for _ in range(n):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, rmax + 1)
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.ogrid[y0:y1, x0:x1]
        u[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return u


# ---- sizes and hole shapes against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 0])
def test_single_pixel_raster(dev, order):
    z = np.full((1, 1), 901.5, np.float32)
    g = np.full((1, 1), 903.0, np.float32)
    o, info, _ = _check(z, g, order=order)                                   # known: comes back as it is
    assert o[0, 0] == z[0, 0] and info["ring"] == info["interior"] == info["unfilled"] == 0 and info["cycles"] == 0
    o, info, _ = _check(z, g, np.zeros((1, 1), np.float32), order=order)     # a filled hole with nothing known: unchanged
    assert o[0, 0] == g[0, 0] and info["interior"] == 1
    o, info, _ = _check(np.full((1, 1), np.nan, np.float32), np.full((1, 1), np.nan, np.float32), order=order)
    assert np.isnan(o[0, 0]) and info["unfilled"] == 1


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("H,W", [(1, 700), (700, 1)])
def test_lines(dev, H, W, order):
    z = RO.terrain(H, W, 1)
    n = max(H, W)
    k = np.ones(n, bool)
    k[:30] = False                                      # touches the first end
    k[200:380] = False                                  # an interior run
    k[n - 9:] = False                                   # touches the other end
    k[400:600:37] = False                               # single pixels
    k[450:452] = False
    k = k.reshape(H, W)
    g = _fill(z, 2, k)
    g.reshape(-1)[250:270] = np.nan                     # an unfilled stretch inside the run
    _check(z, g, k.astype(np.float32), order=order)


@pytest.mark.parametrize("order", [1, 0])
def test_discs_strokes_edges_and_corner_37x53(dev, order):
    H, W = 37, 53
    z = RO.terrain(H, W, 2)
    k = ~(VO.disc(H, W, 18, 26, 9) | VO.disc(H, W, 6, 45, 3))
    _check(z, _fill(z, 3, k), k.astype(np.float32), order=order)
    k = np.ones((H, W), bool)
    k[5, 3:50] = False                                  # 1-px strokes
    k[8:34, 40] = False
    k[np.arange(10, 30), np.arange(10, 30)] = False     # a diagonal stroke (4-disconnected pixels)
    o, info, _ = _check(z, _fill(z, 4, k), k.astype(np.float32), order=order)
    assert info["interior"] == 0 and info["cycles"] == 0
    k = np.ones((H, W), bool)
    k[:9, :12] = False                                  # a corner: two raster edges
    k[15:25, W - 6:] = False                            # the right edge
    k[H - 1, 20:33] = False                             # a stroke on the bottom edge
    k[H - 5:, :4] = False                               # another corner
    _check(z, _fill(z, 5, k), k.astype(np.float32), order=order)


@pytest.mark.parametrize("order", [1, 0])
def test_special_pixels_and_unfilled_patches_257x129(dev, order):
    H, W = 257, 129
    z = RO.terrain(H, W, 3)
    z0 = z.copy()
    rng = np.random.default_rng(3)
    z[rng.random((H, W)) < 0.02] = np.nan
    z[rng.random((H, W)) < 0.01] = np.inf
    z[rng.random((H, W)) < 0.01] = -np.inf
    z[rng.random((H, W)) < 0.02] = -9999.0
    z[30:60, 20:45] = -9999.0
    z[200:230, 60:110] = np.nan
    m = np.ones((H, W), np.float32)
    m[80:100, 60:90] = 0
    m[150:153, :] = 0
    m[:, 100] = 0
    z[38:43, 75:80] = z0[38:43, 75:80]                  # a known 5 x 5 block around a -0.0: no ring target reads the zero
    z[40, 77] = -0.0
    k = VO.known_mask(z, m, -9999.0)
    assert k[38:43, 75:80].all()
    g = _fill(z, 6, k)
    g[35:50, 25:40] = np.nan                            # unfilled patches inside the holes
    g[205:215, 70:100] = np.inf
    g[85:90, 60:90] = -np.inf
    o, info, _ = _check(z, g, m, nodata=-9999.0, order=order)
    assert _bits(o[40, 77]) == _bits(np.float32(-0.0)) and info["unfilled"] > 0
    # a NaN nodata is ignored: the -9999 pixels are known, and come back
    from mvp_gan.src.seam_correct import correct_seams
    a, ia = correct_seams(z, g, m, nodata=float("nan"), order=order)
    b, ib = correct_seams(z, g, m, order=order)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and ia == ib
    # (counted over the known pixels only: with order 0 a ring pixel whose known neighbours all hold -9999 has that as target)
    kn = VO.known_mask(z, m, None)
    an = a.cpu().numpy()
    assert np.array_equal(_bits(an[kn]), _bits(z[kn]))
    assert int((an[kn] == -9999.0).sum()) == int(((z == -9999.0) & (m != 0)).sum()) > 0


@pytest.mark.parametrize("order", [1, 0])
def test_many_small_holes_1500x2100(dev, order):
    H, W = 1500, 2100
    z = RO.terrain(H, W, 6)
    u = _discs(H, W, 6, 400, 19)
    rng = np.random.default_rng(7)
    for _ in range(60):                                 # strokes
        y, x0 = rng.integers(0, H), rng.integers(0, W - 60)
        u[y, x0:x0 + 60] = True
    u[:14, :20] = True                                  # a corner and two edges
    u[700:730, W - 9:] = True
    u[H - 6:, 900:960] = True
    z[3, 1000] = -0.0
    u[:8, 990:1010] = False                             # the -0.0 is known and no target reads it
    g = _fill(z, 8, ~u)
    g[np.where(u & (rng.random((H, W)) < 0.002))] = np.nan     # scattered unfilled pixels
    o, info, _ = _check(z, g, (~u).astype(np.float32), order=order)
    assert _bits(o[3, 1000]) == _bits(np.float32(-0.0))
    assert info["cycles"] >= 1 and info["interior"] > 0


def test_no_holes_at_all(dev):
    z = RO.terrain(120, 90, 9)
    z[5, 5] = -0.0
    o, info, _ = _check(z, _fill(z, 9))
    assert np.array_equal(_bits(o), _bits(z))
    assert info == {"ring": 0, "interior": 0, "unfilled": 0, "order": 1, "max_delta": 0.0, "cycles": 0, "change": 0.0,
                    "tol": 0.0, "converged": True}


def test_nothing_known(dev):
    z = RO.terrain(120, 90, 10)
    g = _fill(z, 10)
    g[30:40, 20:50] = np.nan
    g[0, 0] = -0.0
    o, info, _ = _check(z, g, np.zeros(z.shape, np.float32))
    f = np.isfinite(g)
    assert np.array_equal(_bits(o[f]), _bits(g[f])) and np.isnan(o[~f]).all()      # the fill, unchanged
    assert info["ring"] == 0 and info["interior"] == int(f.sum()) and info["cycles"] == 0
    o, info, _ = _check(np.full(z.shape, np.nan, np.float32), g)
    assert np.array_equal(_bits(o[f]), _bits(g[f]))


def test_tol_and_max_cycles_are_passed_to_the_solver(dev):
    from mvp_gan.src.seam_correct import correct_seams
    z = RO.terrain(200, 200, 11)
    k = ~VO.disc(200, 200, 100, 100, 60)
    g = _fill(z, 11, k)
    _, info = correct_seams(z, g, k.astype(np.float32), tol=0.0, max_cycles=2)
    assert info["cycles"] == 2 and not info["converged"] and info["tol"] == 0.0
    _, info = correct_seams(z, g, k.astype(np.float32), tol=10.0)
    assert info["cycles"] == 1 and info["converged"] and info["tol"] == 10.0


# ---- planar exactness against the closed form -----------------------------------------------------------------------
def test_order_1_is_exact_on_a_plane_4096(dev):
    """z = 900 + x / 4 - y / 8 is exact in fp32; the fill is the plane plus a discrete-harmonic error of metres inside discs of
    radius up to 300.  Order 1 continues the plane exactly onto the ring, and the harmonic extension of a discrete-harmonic
    field is that field, so the result is the plane.  Bound: the oracle bound above, plus twice the rounding of the fill to
    fp32 (once in the ring's delta, once in the final add)."""
    from mvp_gan.src.seam_correct import correct_seams
    H = W = 4096
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    plane = 900.0 + x / 4 - y / 8
    z = plane.astype(np.float32)
    assert np.array_equal(z.astype(np.float64), plane)
    u = VO.disc(H, W, 1200, 1300, 300) | VO.disc(H, W, 3000, 2900, 250) | VO.disc(H, W, 2500, 900, 300)
    for cy, cx, r in ((600, 3300, 120), (3600, 400, 60), (2000, 2000, 8), (330, 330, 300)):
        u |= VO.disc(H, W, cy, cx, r)
    xs, ys = (x - 2048) / 2048, (y - 2048) / 2048
    e = 2.5 + 6 * xs - 4 * ys + 9 * (xs * xs - ys * ys)
    g64 = plane + e
    g = np.where(u, g64, np.nan).astype(np.float32)
    out, info = correct_seams(z, g, (~u).astype(np.float32), order=1)
    assert info["converged"] and info["ring"] + info["interior"] == int(u.sum()) and info["unfilled"] == 0, info
    o = out.cpu().numpy()
    err = float(np.abs(o.astype(np.float64) - plane)[u].max())
    data = float(np.abs(g.astype(np.float64) - g64)[u].max())
    ring = SO.classify(z, g, (~u).astype(np.float32))[1]
    D = (plane - g64)[ring]                            # the delta raster's fixed pixels: the ring, and 0 at the known pixels
    bound = SOLVER_BOUND * float(max(D.max(), 0.0) - min(D.min(), 0.0)) + ROUND_BOUND * float(np.abs(g64[u]).max()) + 2 * data
    print(f"plane 4096: max error {err:.3g} m, bound {bound:.3g} m, ratio {err / bound:.3f} "
          f"({err / (bound - 2 * data):.3f} of the bound without the fill's rounding), info {info}")
    assert err <= bound, (err, bound, info)
    assert np.array_equal(_bits(o[~u]), _bits(z[~u]))
    # order 0 is not exact here: the two orders cannot be swapped
    out0, info0 = correct_seams(z, g, (~u).astype(np.float32), order=0)
    assert float(np.abs(out0.cpu().numpy().astype(np.float64) - plane)[u].max()) > 10 * bound


# ---- inpaint_raster(seam="harmonic") --------------------------------------------------------------------------------
def _holed(H, W, seed, frac=0.12):
    z = RO.terrain(H, W, seed)
    hole = RO.disc_holes(H, W, frac, seed + 1, rmin=6, rmax=30)
    return z, (~hole).astype(np.float32)


def test_inpaint_seam_is_correct_seams_of_the_plain_output(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.seam_correct import correct_seams
    z, m = _holed(640, 768, 20)
    z[100:130, 300:360] = -9999.0
    kw = dict(nodata=-9999.0, window=256, overlap=32, batch=8)
    out0, info0 = inpaint_raster(G, z, m, **kw)
    outn, infon = inpaint_raster(G, z, m, seam=None, **kw)
    assert np.array_equal(_bits(outn.cpu().numpy()), _bits(out0.cpu().numpy()))
    assert list(infon) == list(info0) and infon == info0 and "seam" not in info0
    for order in (1, 0):
        outs, infos = inpaint_raster(G, z, m, seam="harmonic", seam_order=order, **kw)
        ref, rinfo = correct_seams(z, out0, m, nodata=-9999.0, order=order)
        assert np.array_equal(_bits(outs.cpu().numpy()), _bits(ref.cpu().numpy()))
        assert infos["seam"] == rinfo and rinfo["order"] == order and rinfo["converged"] and rinfo["ring"] > 0
        assert {k: v for k, v in infos.items() if k != "seam"} == info0
    outd, infod = inpaint_raster(G, z, m, seam="harmonic", **kw)                  # the default order is 1
    assert infod["seam"]["order"] == 1
    # the ring now sits on its target: the step at the hole outlines is gone
    k = VO.known_mask(z, m, -9999.0)
    r8 = SO.ring8(k, ~k)
    rm = lambda a: math.sqrt(float(((a.cpu().numpy().astype(np.float64) - z)[r8 & (z != -9999.0)] ** 2).mean()))
    print(f"ring RMSE against the truth: {rm(out0):.3f} m -> {rm(outd):.3f} m")
    with pytest.raises(ValueError, match="seam"):
        inpaint_raster(G, z, m, seam="poisson", **kw)
    with pytest.raises(ValueError, match="seam_order"):
        inpaint_raster(G, z, m, seam="harmonic", seam_order=2, **kw)


def test_inpaint_seam_uses_the_keep_mask_of_objects(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.object_mask import ObjectSpec, object_mask
    from mvp_gan.src.seam_correct import correct_seams
    from tests import objmask_oracle as OR
    z, _ = OR.scene(1024, 1024, 3, buildings=50, trees=100)
    z[700:730, 100:180] = -9999.0
    spec = ObjectSpec()
    _, keep, _ = object_mask(z, nodata=-9999.0, cellsize=1.0, spec=spec)
    kw = dict(nodata=-9999.0, window=256, overlap=32, objects=spec, cellsize=1.0)
    out0, _ = inpaint_raster(G, z, **kw)
    outs, infos = inpaint_raster(G, z, seam="harmonic", **kw)
    ref, rinfo = correct_seams(z, out0, keep, nodata=-9999.0)
    assert torch.equal(outs, ref) and infos["seam"] == rinfo and rinfo["ring"] > 0 and "objects" in infos


def test_seam_runs_before_the_fallback(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H = W = 320
    z = RO.terrain(H, W, 21)
    m = np.ones((H, W), np.float32)
    m[60:230, 60:230] = 0                               # its middle is reached by no 64-px window
    kw = dict(window=64, overlap=8, batch=8)
    outs, infos = inpaint_raster(G, z, m, seam="harmonic", **kw)
    outf, infof = inpaint_raster(G, z, m, seam="harmonic", fallback="laplace", **kw)
    os_, of = outs.cpu().numpy(), outf.cpu().numpy()
    fin = np.isfinite(os_)
    assert infos["unfilled"] == int((~fin).sum()) > 0 and infos["seam"]["unfilled"] == infos["unfilled"]
    assert infof["unfilled"] == 0 and np.isfinite(of).all()
    assert np.array_equal(_bits(of[fin]), _bits(os_[fin]))       # known and corrected GAN pixels keep their values
    assert infof["seam"] == infos["seam"] and infof["fallback"]["pixels"] == infos["unfilled"]
    assert infof["fallback"]["converged"] and list(infof).index("seam") < list(infof).index("fallback")


# ---- evaluate_raster(seam="harmonic") -------------------------------------------------------------------------------
def test_evaluate_seam(dev, G):
    from mvp_gan.src.evaluate_raster import evaluate_raster
    H, W, c = 768, 1024, 1.0
    z = RO.terrain(H, W, 22)
    kw = dict(cellsize=c, split="test", block=512, tile=128, seed=2, window=256, overlap=32, batch=8)
    rep0, pred0 = evaluate_raster(G, z, **kw)
    repn, predn = evaluate_raster(G, z, seam=None, **kw)
    assert json.dumps(repn) == json.dumps(rep0) and torch.equal(predn, pred0) and "seam" not in rep0
    rep, pred = evaluate_raster(G, z, seam="harmonic", **kw)
    assert set(rep) == set(rep0) | {"seam"} and set(rep["seam"]) == INFO_KEYS
    assert rep["seam"] == rep["inpaint"]["seam"] and rep["seam"]["converged"] and rep["seam"]["ring"] > 0
    assert {k: v for k, v in rep["inpaint"].items() if k != "seam"} == rep0["inpaint"]
    assert rep["pixels"] == rep0["pixels"]
    r0, r1 = rep0["ring"]["rmse"], rep["ring"]["rmse"]
    print(f"ring RMSE {r0:.3f} -> {r1:.3f} m, height RMSE {rep0['height']['rmse']:.3f} -> {rep['height']['rmse']:.3f} m")
    assert math.isfinite(r1) and r1 < r0
    rep2, _ = evaluate_raster(G, z, seam="harmonic", **kw)
    assert json.dumps(rep2) == json.dumps(rep)
    with pytest.raises(ValueError, match="seam"):
        evaluate_raster(G, z, seam="poisson", **kw)


# ---- CLIs -----------------------------------------------------------------------------------------------------------
def _write_asc(path, a, c, nodata=None):
    from mvp_gan.src.asc import write_asc
    hdr = [("ncols", str(a.shape[1])), ("nrows", str(a.shape[0])), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", str(c))]
    if nodata is not None:
        hdr.append(("NODATA_value", str(nodata)))
    write_asc(path, a, hdr)


def test_clis(dev, G, tmp_path):
    from mvp_gan.src.asc import read_asc
    from mvp_gan.src.seam_correct import correct_seams
    H, W, c = 300, 420, 2.0
    z = RO.terrain(H, W, 23)
    hole = RO.disc_holes(H, W, 0.1, 24, rmin=5, rmax=25)
    zh = np.where(hole, np.float32(-9999.0), z)
    g = _fill(z, 25)
    g[hole & (np.arange(W)[None, :] > 380)] = np.nan   # the holes at the right edge stay unfilled
    dem, fil = str(tmp_path / "dem.asc"), str(tmp_path / "filled.asc")
    _write_asc(dem, zh, c, -9999)
    _write_asc(fil, g, c, -9999)
    env = dict(os.environ)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda mod, args: subprocess.run([sys.executable, "-m", f"mvp_gan.src.{mod}", "--dem", dem] + args, cwd=cwd,
                                           capture_output=True, text=True, timeout=600, env=env)
    # seam_correct
    out = str(tmp_path / "seam.asc")
    r = run("seam_correct", ["--filled", fil, "--out", out, "--order", "0"])
    assert r.returncode == 0, r.stderr
    assert "ring /" in r.stdout and "interior pixels" in r.stdout and "max_delta" in r.stdout and "cycles" in r.stdout
    assert "converged True" in r.stdout and "warning" not in r.stdout
    zr, _ = read_asc(dem)
    gr, _ = read_asc(fil)
    gr = np.where(gr == np.float32(-9999.0), np.float32(np.nan), gr)
    ref, info = correct_seams(zr, gr, nodata=-9999.0, order=0)
    a, _ = read_asc(out)
    refn = ref.cpu().numpy()
    assert info["unfilled"] > 0 and info["ring"] > 0
    assert np.array_equal(_bits(a), _bits(np.where(np.isnan(refn), np.float32(-9999.0), refn)))
    r = run("seam_correct", ["--filled", fil, "--out", out, "--max-cycles", "1", "--tol", "0"])
    assert r.returncode == 0 and "converged False" in r.stdout and "warning: not converged" in r.stdout, r.stdout
    # inpaint_raster --seam
    ck = str(tmp_path / "g.pth")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    ip = str(tmp_path / "inp.asc")
    r = run("inpaint_raster", ["--checkpoint", ck, "--out", ip, "--window", "128", "--overlap", "16", "--seam", "harmonic",
                               "--seam-order", "0"])
    assert r.returncode == 0, r.stderr
    assert "seam harmonic:" in r.stdout and "converged True" in r.stdout and " 0 holes left unfilled" in r.stdout
    a, _ = read_asc(ip)
    assert np.isfinite(a).all() and not (a == -9999.0).any()
    # evaluate_raster --seam
    js = str(tmp_path / "r.json")
    r = run("evaluate_raster", ["--checkpoint", ck, "--json", js, "--block", "160", "--tile", "80", "--window", "128",
                                "--overlap", "16", "--seam", "harmonic"])
    assert r.returncode == 0, r.stderr
    assert "seam harmonic:" in r.stdout and "ring RMSE" in r.stdout
    rep = json.load(open(js))
    assert set(rep["seam"]) == INFO_KEYS and rep["seam"]["converged"]
