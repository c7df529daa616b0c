"""GPU checks of the raster resampling (csrc/resample.hip, mvp_gan/src/resample.py) against the fp64
oracle in tests/resample_oracle.py.

The known masks must equal the oracle's at every pixel; every mask bit is decided in integers, so there is nothing to
tolerate.  Value bound, per pixel, with u = 2^-24 (half an fp32 ulp, relative), n the taps of that pixel's formula (the
footprint for the area kernel, 16 or 4 for the interpolation), R the range of the known taps it read and max|z| the largest
known |z| of the source raster:

    |out - oracle| <= K u (max|z| + n R),   K = 8.

The count behind it.  Area: d_k = z_k - z0 is one rounding, <= u R (exact within a binade); the n fused multiply-adds of
num round once each at a partial sum of at most (sum w) R, and carry the d errors through with the same total weight:
(n + 1) u (sum w) R; the weights and sum w are integers below 2^24, exact in fp32; the division by sum w rounds once at a
quotient of at most R; the final add z0 + q rounds once at <= max|z| + R.  Together u (max|z| + (n + 3) R), inside the bound for
every n >= 1.  Interpolation, bicubic: each weight is the exact rational rounded to fp32 (u, relative), and the absolute
Catmull-Rom weights sum to at most 1.25 per axis, 1.5625 over the 16 taps; the 16 differences (u R each) and the two sets of
weight roundings cost 1.5625 u R apiece; the 4 fused multiply-adds of each row round at partial sums of at most 1.25 R and enter
the column sum with weight 1.25, those of the column sum round at up to 1.5625 R: 6.25 u R each; the final add rounds at
max|z| + 1.5625 R.  Together u (max|z| + about 19 R), against the 128 R the bound allows at n = 16.  Bilinear: 4 differences, 4
fused multiply-adds with exact integer weights, one division, one add: u (max|z| + 7 R) against 32 R.
K = 8 therefore covers every rounding listed in the issue with room; no case needed a larger one.  The oracle's own fp64
rounding is eight orders of magnitude below u.

A footprint whose known taps all hold one value (R == 0) must return that value bit for bit.

Also: the 1500 x 2100 raster at 10/3 and 3/10, the return trip with its pass-through, determinism, inpaint_raster /
evaluate_raster / RasterWindowLoader with model_cellsize, and the CLIs."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import raster_oracle as RO
from tests import resample_oracle as XO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8
U = 2.0 ** -24
NODATA = -9999.0
AREA_SCALES = [(2, 1), (3, 1), (5, 2), (10, 3), (16, 1)]
INTERP_SCALES = [(1, 2), (2, 3), (3, 10), (1, 4)]
SHAPES = [(203, 317), (257, 130)]


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


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


_SCENES = {}


def _scene(H, W):
    """Terrain within one binade (850 .. 970 m) with holes in discs, NaN, +-inf and nodata pixels, a mask, an all-hole region
    wider than any footprint, and a region of one repeated value (with holes of its own)."""
    if (H, W) not in _SCENES:
        z = RO.terrain(H, W, H + W)
        rng = np.random.default_rng(H * W)
        z[rng.random((H, W)) < 0.02] = np.nan
        z[rng.random((H, W)) < 0.005] = np.inf
        z[rng.random((H, W)) < 0.005] = -np.inf
        z[rng.random((H, W)) < 0.02] = NODATA
        z[H - 60:H - 10, 20:75] = np.float32(903.25)                # a lake
        z[H - 40:H - 30, 30:50] = np.nan
        z[H - 55, 22:70:3] = NODATA
        m = (~RO.disc_holes(H, W, 0.15, H, rmin=2, rmax=12)).astype(np.float32)
        m[30:90, W - 70:W - 5] = 0                                   # wider than a 16 x 16 footprint
        m[:, 101] = 0
        m[0:3, 0:9] = 0                                              # a corner
        _SCENES[H, W] = (z, m)
    return _SCENES[H, W]


_ORACLE = {}


def _oracle(kind, H, W, p, q):
    """Computed once and shared; never written to."""
    key = (kind, H, W, p, q)
    if key not in _ORACLE:
        z, m = _scene(H, W)
        _ORACLE[key] = XO.area(z, m, NODATA, p, q, Fraction(1, 2)) if kind == "area" else XO.interp(z, m, NODATA, p, q)
    return _ORACLE[key]


def _compare(o, k, n_nan, ref, zmax, what):
    """GPU raster o, mask k and NaN counter against an oracle dict -> the worst error / bound."""
    kn = ref["known"]
    assert o.shape == kn.shape == k.shape, (o.shape, kn.shape)
    assert np.array_equal(k != 0, kn), f"{what}: {int(((k != 0) != kn).sum())} mask pixels differ"
    assert np.isin(k, (0.0, 1.0)).all()
    assert np.isnan(o[~kn]).all() and np.isfinite(o[kn]).all()
    assert n_nan == int((~kn).sum())
    if not kn.any():
        return 0.0
    err = np.abs(o.astype(np.float64) - ref["value"])[kn]
    bound = (K * U * (zmax + ref["n"] * ref["R"]))[kn]
    ratio = float((err / bound).max())
    print(f"{what}: {int(kn.sum())} known / {int((~kn).sum())} unknown, max error {err.max():.3g} m, worst error / bound {ratio:.3f}")
    assert (err <= bound).all(), (what, float(err.max()), ratio)
    flat = kn & (ref["R"] == 0) & ~ref["passed"]
    assert np.array_equal(_bits(o[flat]), _bits(ref["value"][flat].astype(np.float32)))      # constants bit for bit
    return ratio


def _zmax(z, m=None, nodata=None):
    k = XO.known(np.asarray(z, np.float32), m, nodata)
    return float(np.abs(np.asarray(z, np.float64)[k]).max())


# ---- the kernels against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("p,q", AREA_SCALES)
def test_area_against_oracle(dev, H, W, p, q):
    from tg_hip import ops as O
    z, m = _scene(H, W)
    ref = _oracle("area", H, W, p, q)
    out, km, nn = O.resample_area(_t(z, dev), _t(m, dev), NODATA, p, q, 1, 2)
    o = out.cpu().numpy()
    _compare(o, km.cpu().numpy(), int(nn.item()), ref, _zmax(z, m, NODATA), f"area {p}/{q} {H}x{W}")
    assert ref["known"].any() and (~ref["known"]).any()
    lake = ref["known"] & (ref["R"] == 0) & (ref["n"] > 1)
    assert lake.any() and (o[lake] == np.float32(903.25)).any()
    out2, km2, nn2 = O.resample_area(_t(z, dev), _t(m, dev), NODATA, p, q, 1, 2)                 # determinism
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and torch.equal(km2, km) and torch.equal(nn2, nn)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("p,q", INTERP_SCALES)
def test_interp_against_oracle(dev, H, W, p, q):
    from tg_hip import ops as O
    z, m = _scene(H, W)
    ref = _oracle("interp", H, W, p, q)
    out, km, nn = O.resample_interp(_t(z, dev), _t(m, dev), NODATA, p, q)
    o = out.cpu().numpy()
    _compare(o, km.cpu().numpy(), int(nn.item()), ref, _zmax(z, m, NODATA), f"interp {p}/{q} {H}x{W}")
    kn = ref["known"]
    assert (kn & ref["bicubic"]).any() and (kn & ~ref["bicubic"]).any() and (~kn).any()          # both formulas ran
    lake = kn & (ref["R"] == 0)
    assert lake.any() and (o[lake] == np.float32(903.25)).any()
    out2, km2, nn2 = O.resample_interp(_t(z, dev), _t(m, dev), NODATA, p, q)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and torch.equal(km2, km) and torch.equal(nn2, nn)


def test_coverage_threshold_is_exact(dev):
    """Half a footprint known at scale 2 is a tie at min_coverage 0.5: known; just above it, unknown."""
    from tg_hip import ops as O
    z, _ = _scene(203, 317)
    z = np.where(np.isfinite(z) & (z != NODATA), z, np.float32(900.0))
    m = np.ones(z.shape, np.float32)
    m[:, 0::2] = 0                                                   # every footprint exactly half known
    m[50:60, :] = 0
    for cov, want in ((Fraction(1, 2), True), (Fraction(501, 1000), False), (Fraction(1, 1000), True), (Fraction(1), False)):
        out, km, nn = O.resample_area(_t(z, dev), _t(m, dev), None, 2, 1, cov.numerator, cov.denominator)
        ref = XO.area(z, m, None, 2, 1, cov)
        _compare(out.cpu().numpy(), km.cpu().numpy(), int(nn.item()), ref, _zmax(z, m), f"coverage {cov}")
        assert bool(ref["known"][10, 10]) == want and not ref["known"][27, 10]


def test_scale_1_and_unaligned_views(dev):
    """p = q = 1 returns the input with its unknown pixels NaN; a raster that does not start on a 16-byte boundary takes the
    pixel-wide staging path and gives the same bits."""
    from tg_hip import ops as O
    z, m = _scene(257, 130)
    out, km, nn = O.resample_area(_t(z, dev), _t(m, dev), NODATA, 1, 1)
    k = XO.known(z, m, NODATA)
    o = out.cpu().numpy()
    assert np.array_equal(_bits(o[k]), _bits(z[k])) and np.isnan(o[~k]).all() and int(nn.item()) == int((~k).sum())
    assert np.array_equal(km.cpu().numpy() != 0, k)
    zt, mt = _t(z, dev), _t(m, dev)
    o0, k0, n0 = O.resample_area(zt, mt, NODATA, 1, 1, count_only=True)                          # no raster written
    assert o0 is None and k0 is None and int(n0.item()) == int(O.raster_count_unknown(zt, mt, NODATA).item()) == int((~k).sum())
    assert int(O.raster_count_unknown(zt, None, None).item()) == int((~np.isfinite(z)).sum())
    a, ka, na = O.resample_area(zt, mt, NODATA, 10, 3)
    for shift in (1, 2, 3):
        buf_z = torch.empty(z.size + 4, dtype=torch.float32, device=dev)
        buf_m = torch.empty(z.size + 4, dtype=torch.float32, device=dev)
        zs, ms = buf_z[shift:shift + z.size].view(z.shape), buf_m[shift:shift + z.size].view(z.shape)
        zs.copy_(zt), ms.copy_(mt)
        assert zs.data_ptr() % 16 != 0
        b, kb, nb = O.resample_area(zs, ms, NODATA, 10, 3)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ka, kb) and torch.equal(na, nb)


def test_large_raster_1500x2100(dev):
    """Many workgroups per axis and output widths that are no multiple of the tile: 450 x 630 at 10/3 against the whole
    oracle, 5000 x 7000 at 3/10 against the oracle on bands of rows and of columns (first, last, around tile borders), its
    mask at every pixel against the rule restated: known iff source pixel floor((I + 1/2) p / q), clamped, is."""
    from tg_hip import ops as O
    H, W = 1500, 2100
    z = RO.terrain(H, W, 6)
    rng = np.random.default_rng(6)
    m = (~RO.disc_holes(H, W, 0.2, 7, rmin=3, rmax=40)).astype(np.float32)
    z[rng.random((H, W)) < 0.01] = np.nan
    z[700:760, 1000:1100] = np.float32(900.5)
    zt, mt = _t(z, dev), _t(m, dev)
    zmax = _zmax(z, m)
    out, km, nn = O.resample_area(zt, mt, None, 10, 3)
    assert tuple(out.shape) == (450, 630)
    _compare(out.cpu().numpy(), km.cpu().numpy(), int(nn.item()), XO.area(z, m, None, 10, 3), zmax, "area 10/3 1500x2100")
    out, km, nn = O.resample_interp(zt, mt, None, 3, 10)
    assert tuple(out.shape) == (5000, 7000)
    o, k = out.cpu().numpy(), km.cpu().numpy()
    assert int(nn.item()) == int(np.isnan(o).sum()) and np.array_equal(k != 0, np.isfinite(o))
    iy = np.minimum((2 * np.arange(5000) + 1) * 3 // 20, H - 1)
    ix = np.minimum((2 * np.arange(7000) + 1) * 3 // 20, W - 1)
    want = XO.known(z, m)[iy][:, ix]
    assert np.array_equal(k != 0, want), f"{int(((k != 0) != want).sum())} mask pixels differ"
    rows = np.unique(np.concatenate([np.arange(0, 6), np.arange(2497, 2503), np.arange(4994, 5000), rng.integers(0, 5000, 12)]))
    cols = np.unique(np.concatenate([np.arange(0, 6), np.arange(3581, 3587), np.arange(6994, 7000), rng.integers(0, 7000, 12)]))
    ref = XO.interp(z, m, None, 3, 10, rows=rows)
    _compare(o[rows], k[rows], int((~ref["known"]).sum()), ref, zmax, "interp 3/10 1500x2100, row bands")
    ref = XO.interp(z, m, None, 3, 10, cols=cols)
    _compare(o[:, cols], k[:, cols], int((~ref["known"]).sum()), ref, zmax, "interp 3/10 1500x2100, column bands")


# ---- the return trip ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", [(2, 1), (10, 3), (16, 1), (1, 2), (3, 10), (1, 4)])
def test_return_trip(dev, p, q):
    """Forward, then back onto the native grid: known pixels carry the input's bits (a -0.0 and a pixel equal to a nodata value
    that is not in use among them), holes follow the oracle, NaN is counted and present where the working surface is missing."""
    from mvp_gan.src.resample import resample_back, resample_raster
    H, W = 203, 317
    z = RO.terrain(H, W, 31)
    m = (~RO.disc_holes(H, W, 0.12, 32, rmin=2, rmax=9)).astype(np.float32)
    m[60:150, 40:160] = 0                                            # its middle has no working surface at any scale
    z[20, 300] = -0.0
    z[21, 300] = np.float32(999.0)                                   # would be a hole under nodata = 999, which is not given
    z[5, 5] = np.nan
    m[18:24, 296:306] = 1
    work, wk, info = resample_raster(z, m, cellsize=1.0, target_cellsize=float(Fraction(p, q)), min_coverage=0.25)
    assert info["scale"] == f"{p}/{q}" and info["shape"] == (XO.out_size(H, p, q), XO.out_size(W, p, q))
    assert info["known"] + info["unknown"] == work.numel() and info["unknown"] == int(torch.isnan(work).sum())
    out, nn = resample_back(work, z, m, scale=info["scale"])
    o = out.cpu().numpy()
    w = work.cpu().numpy()
    ref = XO.back(w, z, m, None, p, q)
    k = XO.known(z, m)
    assert o.shape == z.shape and np.array_equal(ref["passed"], k)
    assert np.array_equal(_bits(o[k]), _bits(z[k]))
    assert _bits(o[20, 300]) == _bits(np.float32(-0.0)) and o[21, 300] == np.float32(999.0)
    kn = ref["known"]
    assert np.array_equal(np.isfinite(o), kn) and int(nn.item()) == int((~kn).sum()) > 0 and np.isnan(o[100, 100])
    hole = kn & ~k
    assert hole.any() == (p != 1 or q == 1)            # at 1/2 and 1/4 a native pixel is exactly 4 or 16 working pixels, all holes
    if hole.any():
        zmax = float(np.abs(w[np.isfinite(w)]).max())
        err = np.abs(o.astype(np.float64) - ref["value"])[hole]
        bound = (K * U * (zmax + ref["n"] * ref["R"]))[hole]
        print(f"return {p}/{q}: {int(hole.sum())} hole pixels filled, worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
    out2, nn2 = resample_back(work, z, m, scale=Fraction(p, q))
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32)) and torch.equal(nn2, nn)
    with pytest.raises(ValueError, match="working raster"):
        resample_back(work[:-1], z, m, scale=info["scale"])


def test_resample_raster_nodata_and_identity(dev):
    from mvp_gan.src.resample import resample_raster
    z, m = _scene(203, 317)
    out, km, info = resample_raster(z, m, nodata=NODATA, cellsize=0.3, target_cellsize=1.0)
    ref = _oracle("area", 203, 317, 10, 3)
    _compare(out.cpu().numpy(), km.cpu().numpy(), info["unknown"], ref, _zmax(z, m, NODATA), "resample_raster 0.3 -> 1")
    assert info == {"scale": "10/3", "shape": (61, 96), "cellsize": 1.0, "known": int(ref["known"].sum()),
                    "unknown": int((~ref["known"]).sum())}
    out, km, info = resample_raster(_t(z, dev), _t(m, dev), nodata=NODATA, cellsize=2.0, target_cellsize=2.0)
    k = XO.known(z, m, NODATA)
    o = out.cpu().numpy()
    assert info["scale"] == "1/1" and info["shape"] == z.shape and info["unknown"] == int((~k).sum())
    assert np.array_equal(_bits(o[k]), _bits(z[k])) and np.isnan(o[~k]).all()
    a, _, ia = resample_raster(z, m, nodata=float("nan"), cellsize=1.0, target_cellsize=0.5)      # a NaN nodata is ignored
    b, _, ib = resample_raster(z, m, cellsize=1.0, target_cellsize=0.5)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and ia == ib


# ---- inpaint_raster(model_cellsize=...) -----------------------------------------------------------------------------
def _holed(H, W, seed, frac=0.12):
    z = RO.terrain(H, W, seed)
    hole = RO.disc_holes(H, W, frac, seed + 1, rmin=4, rmax=20)
    return z, (~hole).astype(np.float32)


@pytest.mark.parametrize("c,mc", [(0.5, 1.0), (2.0, 1.0)])
def test_inpaint_is_the_composition_by_hand(dev, G, c, mc):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.resample import resample_back, resample_raster
    z, m = _holed(400, 520, 40)
    z[100:120, 300:340] = NODATA
    kw = dict(window=128, overlap=16, batch=8)
    out, info = inpaint_raster(G, z, m, nodata=NODATA, cellsize=c, model_cellsize=mc, **kw)
    work, wk, winfo = resample_raster(z, m, nodata=NODATA, cellsize=c, target_cellsize=mc)
    ow, iw = inpaint_raster(G, work, **kw)
    ref, nn = resample_back(ow, z, m, nodata=NODATA, scale=winfo["scale"])
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    k = XO.known(z, m, NODATA)
    assert np.array_equal(_bits(out.cpu().numpy()[k]), _bits(z[k]))
    assert list(info) == ["windows", "run", "unfilled", "resample"]
    assert (info["windows"], info["run"], info["unfilled"]) == (iw["windows"], iw["run"], int(nn.item()))
    assert info["resample"] == {"scale": winfo["scale"], "shape": winfo["shape"], "cellsize": mc, "holes": int((~k).sum()),
                                "working_holes": winfo["unknown"], "working_unfilled": iw["unfilled"]}
    assert info["unfilled"] == int(torch.isnan(out).sum()) == 0 and info["run"] > 0


def test_same_cellsize_changes_nothing(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    z, m = _holed(400, 520, 41)
    kw = dict(window=128, overlap=16, batch=8)
    out0, info0 = inpaint_raster(G, z, m, **kw)
    for extra in (dict(cellsize=2.0, model_cellsize=2.0), dict(cellsize=0.5), dict(cellsize=1.0, model_cellsize=1.0 + 1e-9),
                  dict(min_coverage=0.25)):
        out, info = inpaint_raster(G, z, m, **kw, **extra)
        assert torch.equal(out.view(torch.int32), out0.view(torch.int32)) and list(info) == list(info0) and info == info0


def test_inpaint_seam_and_fallback_run_on_the_native_grid(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H, W = 400, 520
    z, m = _holed(H, W, 42)
    m[40:360, 100:420] = 0                                           # a hole no working window reaches the middle of
    k = XO.known(z, m)
    kw = dict(window=64, overlap=8, batch=8, cellsize=0.5, model_cellsize=1.0)
    out, info = inpaint_raster(G, z, m, **kw)
    assert info["unfilled"] > 0 and info["resample"]["working_unfilled"] > 0
    outs, infos = inpaint_raster(G, z, m, seam="harmonic", fallback="laplace", **kw)
    o = outs.cpu().numpy()
    assert np.array_equal(_bits(o[k]), _bits(z[k])) and np.isfinite(o).all() and infos["unfilled"] == 0
    assert list(infos) == ["windows", "run", "unfilled", "resample", "seam", "fallback"]
    sm = infos["seam"]
    assert sm["ring"] + sm["interior"] + sm["unfilled"] == int((~k).sum())      # native pixels
    assert sm["unfilled"] == info["unfilled"] == infos["fallback"]["pixels"] and sm["ring"] > 0 and sm["converged"]
    assert infos["fallback"]["converged"] and infos["resample"] == info["resample"]


def test_a_coarser_model_grid_reaches_a_wide_hole(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H, W = 400, 520
    z = RO.terrain(H, W, 43)
    m = np.ones((H, W), np.float32)
    m[50:350, 110:410] = 0                                           # 300 native pixels wide
    kw = dict(window=128, overlap=16, batch=8)
    _, info = inpaint_raster(G, z, m, **kw)
    assert info["unfilled"] > 0
    out, info4 = inpaint_raster(G, z, m, cellsize=0.5, model_cellsize=2.0, **kw)
    assert info4["unfilled"] == 0 and bool(torch.isfinite(out).all()) and info4["resample"]["scale"] == "4/1"
    assert info4["resample"]["shape"] == (100, 130) and info4["resample"]["holes"] == 300 * 300
    k = m != 0
    assert np.array_equal(_bits(out.cpu().numpy()[k]), _bits(z[k]))
    with pytest.raises(ValueError, match="working grid"):
        inpaint_raster(G, z[:150], m[:150], cellsize=0.5, model_cellsize=2.0, **kw)       # 38 working rows


# ---- evaluate_raster and the training loader ------------------------------------------------------------------------
def test_evaluate_with_model_cellsize(dev, G):
    from mvp_gan.src.evaluate_raster import evaluate_raster
    z = RO.terrain(512, 768, 44)
    kw = dict(cellsize=1.0, split="test", block=256, tile=128, seed=2, window=128, overlap=16, batch=8)
    rep0, pred0 = evaluate_raster(G, z, **kw)
    repn, predn = evaluate_raster(G, z, model_cellsize=1.0, **kw)
    assert json.dumps(repn) == json.dumps(rep0) and torch.equal(predn, pred0)
    rep, pred = evaluate_raster(G, z, model_cellsize=2.0, **kw)
    assert rep["pixels"] == rep0["pixels"] and rep["cells"] == rep0["cells"]      # the holes are cut on the native grid
    assert rep["inpaint"]["resample"]["scale"] == "2/1" and rep["inpaint"]["resample"]["shape"] == (256, 384)
    assert set(rep) == set(rep0) and tuple(pred.shape) == z.shape and np.isfinite(rep["height"]["rmse"])
    print(f"height RMSE {rep0['height']['rmse']:.3f} m native, {rep['height']['rmse']:.3f} m at model_cellsize 2")


def test_loader_with_model_cellsize(dev):
    from mvp_gan.src.resample import resample_raster
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = RO.terrain(600, 640, 45)
    m = np.ones(z.shape, np.float32)
    m[200:230, 100:500] = 0
    z[400:410, 300:330] = NODATA
    work, _, info = resample_raster(z, m, nodata=NODATA, cellsize=0.5, target_cellsize=1.0)
    kw = dict(window=64, batch_size=4, steps_per_epoch=2, seed=5, device=dev)
    A = RasterWindowLoader(z, m, nodata=NODATA, cellsize=0.5, model_cellsize=1.0, **kw)
    B = RasterWindowLoader(work.cpu().numpy(), **kw)
    assert (A.H, A.W) == (B.H, B.W) == info["shape"] == (300, 320) and A.info == B.info
    assert A.info["valid_fraction"] < 1.0
    for a, b in zip(list(A), list(B)):
        assert set(a) == set(b)
        for key in a:
            assert torch.equal(a[key], b[key]), key


def test_evaluate_and_loader_pass_min_coverage_on(dev, G):
    from mvp_gan.src.evaluate_raster import evaluate_raster
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.resample import resample_raster
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = RO.terrain(300, 340, 48)
    m = np.ones(z.shape, np.float32)
    m[100:140, 200:260:2] = 0                                        # footprints at scale 2 that are exactly half known
    kw = dict(window=64, batch_size=4, steps_per_epoch=1, seed=5)
    infos = {}
    for cov in (0.5, 1.0):
        work, _, winfo = resample_raster(z, m, cellsize=0.5, target_cellsize=1.0, min_coverage=cov)
        A = RasterWindowLoader(z, m, cellsize=0.5, model_cellsize=1.0, min_coverage=cov, device="cuda:0", **kw)
        B = RasterWindowLoader(work.cpu().numpy(), **kw)
        assert A.info == B.info
        infos[cov] = (A.info["valid_fraction"], winfo["unknown"])
    assert infos[0.5] == (1.0, 0) and infos[1.0][0] < 1.0 and infos[1.0][1] == 20 * 30      # the coverage asked for decides
    zt = RO.terrain(256, 384, 49)
    ekw = dict(cellsize=1.0, split="test", block=128, tile=64, seed=2, window=64, overlap=8, batch=8, model_cellsize=2.0)
    rep, pred = evaluate_raster(G, zt, min_coverage=1.0, **ekw)
    rep5, pred5 = evaluate_raster(G, zt, **ekw)
    wh, wh5 = rep["inpaint"]["resample"]["working_holes"], rep5["inpaint"]["resample"]["working_holes"]
    assert wh > wh5 > 0 and rep["pixels"]["holes"] == rep5["pixels"]["holes"] and not torch.equal(pred, pred5)


# ---- CLIs -----------------------------------------------------------------------------------------------------------
def _write_asc(path, a, c, nodata=None):
    from mvp_gan.src.asc import write_asc
    hdr = [("ncols", str(a.shape[1])), ("nrows", str(a.shape[0])), ("xllcorner", "1000"), ("yllcorner", "2000"),
           ("cellsize", str(c))]
    if nodata is not None:
        hdr.append(("NODATA_value", str(nodata)))
    write_asc(path, a, hdr)


def test_clis(dev, G, tmp_path):
    from mvp_gan.src.asc import asc_value, read_asc
    from mvp_gan.src.inpaint_raster import inpaint_raster
    from mvp_gan.src.resample import resample_raster
    H, W, c = 203, 317, 0.3
    z = RO.terrain(H, W, 46)
    hole = RO.disc_holes(H, W, 0.1, 47, rmin=3, rmax=12)
    zh = np.where(hole, np.float32(NODATA), z)
    dem = str(tmp_path / "dem.asc")
    _write_asc(dem, zh, c, -9999)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda mod, args: subprocess.run([sys.executable, "-m", f"mvp_gan.src.{mod}", "--dem", dem] + args, cwd=cwd,
                                           capture_output=True, text=True, timeout=600, env=dict(os.environ))
    # resample
    out = str(tmp_path / "r.asc")
    r = run("resample", ["--cellsize-out", "1.0", "--out", out, "--min-coverage", "0.75"])
    assert r.returncode == 0, r.stderr
    assert "scale 10/3" in r.stdout and "61x96" in r.stdout
    zr, _ = read_asc(dem)
    ref, _, info = resample_raster(zr, nodata=NODATA, cellsize=c, target_cellsize=1.0, min_coverage=0.75)
    a, hdr = read_asc(out)
    refn = ref.cpu().numpy()
    assert info["unknown"] > 0 and f"{info['unknown']} unknown" in r.stdout
    assert np.array_equal(_bits(a), _bits(np.where(np.isnan(refn), np.float32(NODATA), refn)))
    assert (asc_value(hdr, "ncols"), asc_value(hdr, "nrows"), float(asc_value(hdr, "cellsize"))) == ("96", "61", 1.0)
    assert asc_value(hdr, "xllcorner") == "1000" and asc_value(hdr, "NODATA_value") == "-9999"
    assert float(asc_value(hdr, "yllcorner")) == pytest.approx(2000 + H * c - 61 * 1.0, abs=1e-9)
    r = run("resample", ["--cellsize-out", "7", "--out", out])
    assert r.returncode != 0 and "outside" in r.stderr
    # inpaint_raster --model-cellsize
    ck = str(tmp_path / "g.pth")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    ip = str(tmp_path / "inp.asc")
    r = run("inpaint_raster", ["--checkpoint", ck, "--out", ip, "--window", "64", "--overlap", "8", "--model-cellsize", "0.6"])
    assert r.returncode == 0, r.stderr
    assert "working grid 102x159 at cellsize 0.6 (scale 2/1)" in r.stdout and " 0 holes left unfilled" in r.stdout
    a, hdr = read_asc(ip)
    refo, _ = inpaint_raster(G, zr, nodata=NODATA, window=64, overlap=8, cellsize=c, model_cellsize=0.6)
    assert np.array_equal(_bits(a), _bits(refo.cpu().numpy())) and asc_value(hdr, "cellsize") == str(c)
    k = ~hole
    assert np.array_equal(_bits(a[k]), _bits(zr[k]))


def test_train_raster_evaluates_on_the_ground_it_held_out(dev, G, tmp_path):
    """train_raster --model-cellsize --evaluate: block and window are working pixels, the report's block and tile the same
    ground in native pixels (tests/test_resample_cpu.py shows what that guarantees); a combination that has no such native
    plan is refused before the training starts."""
    from mvp_gan.src import train_raster
    z = RO.terrain(256, 384, 50)
    dem, dem2 = str(tmp_path / "dem.asc"), str(tmp_path / "dem2.asc")
    _write_asc(dem, z, 0.5, -9999)
    _write_asc(dem2, z, 0.75, -9999)
    ck, ej = str(tmp_path / "g.pth"), str(tmp_path / "ev.json")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    args = ["--out", str(tmp_path / "ft.pth"), "--init", ck, "--window", "64", "--block", "64", "--batch", "2", "--steps", "1",
            "--val-steps", "1", "--epochs", "1", "--model-cellsize", "1.0", "--evaluate", "--eval-json", ej]
    with pytest.raises(ValueError, match="whole numbers"):            # scale 4/3: a 64 px window is 85 1/3 native pixels
        train_raster.main(["--dem", dem2] + args)
    assert not os.path.exists(tmp_path / "ft.pth")
    r = subprocess.run([sys.executable, "-m", "mvp_gan.src.train_raster", "--dem", dem] + args,
                       cwd=os.path.join(ROOT, "terra-gan_amd"), capture_output=True, text=True, timeout=900, env=dict(os.environ))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "test split: height RMSE" in r.stdout
    ev = json.load(open(ej))
    assert ev["split"] == "test" and ev["tile"] == 128 and ev["block"] == 128 and ev["pixels"]["holes"] > 0
    assert ev["inpaint"]["resample"]["scale"] == "2/1" and ev["inpaint"]["resample"]["shape"] == [128, 192]
