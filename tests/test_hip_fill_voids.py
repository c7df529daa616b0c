"""GPU checks of the harmonic void fill (csrc/voidfill.hip, mvp_gan/src/fill_voids.py) against the fp64 numpy oracle in
tests/vfill_oracle.py and closed-form harmonic fields: max |u - u*| <= 2e-5 x range on every case, known pixels bit for bit,
bitwise determinism, convergence within max_cycles; inpaint_raster(fallback="laplace"), evaluate_raster(baseline="laplace") and
the CLIs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vfill_oracle as VO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5                        # max |u - u*| / range


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


def _terrain(H, W, seed, noise=0.3):
    rng = np.random.default_rng(seed)
    f = VO.harmonic_field(H, W, (120, 4, -3, 2, 1, 0.2), W / 2, H / 2, max(H, W) / 2)
    return (f + 6 * np.sin(np.arange(W) / 17.0)[None, :] * np.cos(np.arange(H) / 23.0)[:, None]
            + rng.normal(0, noise, (H, W))).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check(z, mask=None, nodata=None, max_cycles=50, oracle=True):
    """fill_voids against the oracle; known pixels bit for bit; a second call bitwise equal; -> (out, info)."""
    from mvp_gan.src.fill_voids import fill_voids
    out, info = fill_voids(z, mask, nodata=nodata, max_cycles=max_cycles)
    o = out.cpu().numpy()
    k = VO.known_mask(z, mask, nodata)
    assert info["unknown"] == int((~k).sum())
    assert np.array_equal(_bits(o[k]), _bits(z[k]))
    out2, info2 = fill_voids(z, mask, nodata=nodata, max_cycles=max_cycles)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and info2 == info
    if not k.any():
        assert np.isnan(o).all() and info["unfilled"] == z.size and info["cycles"] == 0
        return o, info
    assert info["unfilled"] == 0 and np.isfinite(o).all()
    assert info["converged"] and info["cycles"] <= max_cycles, info
    if oracle:
        ref = VO.solve(z, k)
        rng = float(z[k].max()) - float(z[k].min())
        err = float(np.abs(o.astype(np.float64) - ref).max())
        assert err <= BOUND * rng + 1e-30, (err, rng, info)
    return o, info


# ---- shapes and geometries against the oracle -----------------------------------------------------------------------
def test_single_pixel_rasters(dev):
    o, info = _check(np.full((1, 1), 7.5, np.float32))
    assert info["cycles"] == 0 and info["unknown"] == 0
    _check(np.full((1, 1), np.nan, np.float32))


@pytest.mark.parametrize("H,W", [(1, 300), (300, 1), (1, 5000), (4000, 1)])
def test_lines(dev, H, W):
    z = _terrain(H, W, 1)
    k = np.ones((H, W), bool)
    n = max(H, W)
    kf = k.reshape(-1)
    kf[: n // 20] = False                              # touches the first end
    kf[n // 3: n // 3 + n // 4] = False                # interior run
    kf[n - 7:] = False                                 # touches the other end
    kf[n // 2 + 50::97] = False                        # single pixels
    _check(z, k)


def test_disc_strokes_checkerboard_37x53(dev):
    H, W = 37, 53
    z = _terrain(H, W, 2)
    k = ~VO.disc(H, W, 18, 26, 9)
    _check(z, k)
    k = np.ones((H, W), bool)
    k[5, 3:50] = False                                 # 1-px strokes
    k[3:34, 40] = False
    k[np.arange(10, 30), np.arange(10, 30)] = False    # a diagonal stroke (4-disconnected pixels)
    _check(z, k)
    yy, xx = np.mgrid[0:H, 0:W]
    _check(z, (yy + xx) % 2 == 0)                      # checkerboard of unknowns


def test_spiral_corridor_and_edges_257x129(dev):
    H, W = 257, 129
    z = _terrain(H, W, 3)
    k = np.ones((H, W), bool)
    y, x, L = 128, 64, 4
    for t in range(20):                                # a 3-px-wide spiral corridor
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[t % 4]
        for _ in range(L):
            if 1 <= y < H - 1 and 1 <= x < W - 1:
                k[y - 1:y + 2, x - 1:x + 2] = False
            y, x = y + dy, x + dx
        L += 3
    _check(z, k)
    k = np.ones((H, W), bool)
    k[:40, :30] = False                                # a corner: two raster edges
    k[200:, 100:] = False
    k[100:140, :12] = False
    _check(z, k)


def test_one_known_pixel_all_known_all_unknown(dev):
    H, W = 257, 129
    z = _terrain(H, W, 4)
    k = np.zeros((H, W), bool)
    k[40, 77] = True
    o, info = _check(z, k, oracle=False)
    assert np.array_equal(_bits(o), _bits(np.full((H, W), z[40, 77])))
    o, info = _check(z)
    assert info["cycles"] == 0 and info["unknown"] == 0 and info["converged"]
    assert np.array_equal(_bits(o), _bits(z))
    _check(z, np.zeros((H, W), np.float32))


def test_nan_inf_and_nodata_are_holes(dev):
    H, W = 120, 97
    z = _terrain(H, W, 5)
    rng = np.random.default_rng(5)
    z[rng.random((H, W)) < 0.03] = np.nan
    z[rng.random((H, W)) < 0.01] = np.inf
    z[rng.random((H, W)) < 0.01] = -np.inf
    z[rng.random((H, W)) < 0.03] = -9999.0
    z[30:50, 20:45] = -9999.0
    m = np.ones((H, W), np.float32)
    m[80:100, 60:90] = 0
    _check(z, m, nodata=-9999.0)
    o, _ = _check(z, m, nodata=float("nan"))           # NaN nodata is ignored: -9999 pixels stay known
    assert (o == -9999.0).sum() == int(((z == -9999.0) & (m != 0)).sum())


def test_many_small_holes_1500x2100(dev):
    H, W = 1500, 2100
    z = _terrain(H, W, 6)
    rng = np.random.default_rng(6)
    u = np.zeros((H, W), bool)
    for _ in range(400):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(2, 20)
        y0, y1, x0, x1 = max(cy - r, 0), min(cy + r + 1, H), max(cx - r, 0), min(cx + r + 1, W)
        yy, xx = np.ogrid[y0:y1, x0:x1]
        u[y0:y1, x0:x1] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    for _ in range(60):                                # strokes
        y, x0 = rng.integers(0, H), rng.integers(0, W - 60)
        u[y, x0:x0 + 60] = True
    _check(z, ~u)


# ---- closed-form fields ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coef", [(300, 40, -25, 30, 12, 3), (-50, -10, 5, 60, -20, -8)])
def test_closed_form_fields_4096(dev, coef):
    from mvp_gan.src.fill_voids import fill_voids
    H = W = 4096
    f = VO.harmonic_field(H, W, coef, 2048, 2048, 2048)
    z = f.astype(np.float32)
    u = VO.disc(H, W, 1200, 1300, 700) | VO.disc(H, W, 3000, 2900, 500) | VO.disc(H, W, 2500, 900, 300)
    for cy, cx, r in ((600, 3300, 120), (3600, 400, 60), (2000, 2000, 8)):
        u |= VO.disc(H, W, cy, cx, r)
    out, info = fill_voids(z, ~u)
    assert info["converged"] and info["unknown"] == int(u.sum()), info
    o = out.cpu().numpy()
    rng = float(z[~u].max()) - float(z[~u].min())
    err = float(np.abs(o[u].astype(np.float64) - f[u]).max())
    # the fp32 data differ from the field by up to half an ulp; by the maximum principle so may the fill
    data = float(np.abs(z.astype(np.float64) - f).max())
    assert err <= BOUND * rng + data, (err, rng, info)
    assert np.array_equal(_bits(o[~u]), _bits(z[~u]))


# ---- inpaint_raster(fallback="laplace") -----------------------------------------------------------------------------
def test_inpaint_fallback_fills_voids_wider_than_a_window(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H = W = 1536
    z = _terrain(H, W, 7)
    m = np.ones((H, W), np.float32)
    m[300:1200, 400:1300] = 0                          # a 900-px void, window 256
    kw = dict(window=256, overlap=32, batch=8)
    out0, info0 = inpaint_raster(G, z, m, **kw)
    assert info0["unfilled"] > 0 and "fallback" not in info0
    out1, info1 = inpaint_raster(G, z, m, fallback="laplace", **kw)
    o0, o1 = out0.cpu().numpy(), out1.cpu().numpy()
    assert info1["unfilled"] == 0 and np.isfinite(o1).all()
    fb = info1["fallback"]
    assert fb["pixels"] == info0["unfilled"] and fb["converged"] and fb["cycles"] >= 1
    fin = np.isfinite(o0)
    assert np.array_equal(_bits(o1[fin]), _bits(o0[fin]))      # known and GAN-filled pixels bit for bit
    assert {k: v for k, v in info1.items() if k not in ("fallback", "unfilled")} == \
        {k: v for k, v in info0.items() if k != "unfilled"}
    out2, info2 = inpaint_raster(G, z, m, fallback="laplace", **kw)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o1)) and info2 == info1


def test_inpaint_fallback_matches_the_oracle(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    H = W = 320
    z = _terrain(H, W, 8)
    m = np.ones((H, W), np.float32)
    m[60:230, 60:230] = 0                              # 2304 px that no 64-px window reaches
    kw = dict(window=64, overlap=8, batch=8)
    out0, info0 = inpaint_raster(G, z, m, **kw)
    o0 = out0.cpu().numpy()
    assert 0 < info0["unfilled"] <= VO.MAX_COMPONENT
    out1, info1 = inpaint_raster(G, z, m, fallback="laplace", **kw)
    o1 = out1.cpu().numpy()
    fin = np.isfinite(o0)
    ref = VO.solve(o0, fin)
    rng = float(o0[fin].max()) - float(o0[fin].min())
    assert float(np.abs(o1.astype(np.float64) - ref).max()) <= BOUND * rng
    assert info1["unfilled"] == 0 and info1["fallback"]["pixels"] == info0["unfilled"]


def test_inpaint_without_holes_left_reports_an_empty_fallback(dev, G):
    from mvp_gan.src.inpaint_raster import inpaint_raster
    z = _terrain(256, 256, 9)
    m = np.ones(z.shape, np.float32)
    m[100:120, 100:130] = 0
    out0, info0 = inpaint_raster(G, z, m, window=128, overlap=16)
    out1, info1 = inpaint_raster(G, z, m, window=128, overlap=16, fallback="laplace")
    assert info0["unfilled"] == 0 and info1["fallback"] == {"pixels": 0, "cycles": 0, "converged": True}
    assert torch.equal(out0, out1)


# ---- evaluate_raster(baseline="laplace") ----------------------------------------------------------------------------
def test_evaluate_baseline(dev, G):
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, terrain_errors
    from mvp_gan.src.fill_voids import fill_voids
    H, W, c = 768, 1024, 1.0
    z = _terrain(H, W, 10)
    z[600:620, 100:200] = np.nan
    kw = dict(cellsize=c, split="test", block=512, tile=128, seed=2, window=256, overlap=32, batch=8)
    rep0, pred0 = evaluate_raster(G, z, **kw)
    rep, pred = evaluate_raster(G, z, baseline="laplace", **kw)
    assert json.dumps({k: v for k, v in rep.items() if k != "baseline"}) == json.dumps(rep0)
    assert torch.equal(pred, pred0)
    h, keep, _ = eval_holes(z, split="test", block=512, tile=128, seed=2)
    bp, finfo = fill_voids(z, keep)
    ref = terrain_errors(z, bp, h, keep, cellsize=c)
    b = rep["baseline"]
    assert b["method"] == "laplace" and b["fill"] == finfo and finfo["converged"]
    assert json.dumps({k: v for k, v in b.items() if k not in ("method", "fill")}) == json.dumps(ref)
    assert b["pixels"] == rep["pixels"] and math.isfinite(b["height"]["rmse"])
    rep2, _ = evaluate_raster(G, z, baseline="laplace", **kw)
    assert json.dumps(rep2) == json.dumps(rep)
    # fallback is passed through: the same holes, inpaint info gains the fallback entry
    rep3, _ = evaluate_raster(G, z, fallback="laplace", **kw)
    assert rep3["inpaint"]["fallback"]["pixels"] == rep0["inpaint"]["unfilled"]


# ---- CLIs -----------------------------------------------------------------------------------------------------------
def _write_asc(path, a, c, nodata=None):
    from mvp_gan.src.asc import write_asc
    hdr = [("ncols", str(a.shape[1])), ("nrows", str(a.shape[0])), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", str(c))]
    if nodata is not None:
        hdr.append(("NODATA_value", str(nodata)))
    write_asc(path, a, hdr)


def test_clis(dev, G, tmp_path):
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.asc import read_asc
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, 11)
    z[100:300, 150:400] = -9999.0                      # wider than a 64-px window
    dem = str(tmp_path / "dem.asc")
    _write_asc(dem, z, c, -9999)
    env = dict(os.environ)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda mod, args: subprocess.run([sys.executable, "-m", f"mvp_gan.src.{mod}", "--dem", dem] + args, cwd=cwd,
                                           capture_output=True, text=True, timeout=600, env=env)
    # fill_voids
    out = str(tmp_path / "filled.asc")
    r = run("fill_voids", ["--out", out])
    assert r.returncode == 0, r.stderr
    assert "void pixels" in r.stdout and "converged True" in r.stdout
    zr, _ = read_asc(dem)
    f, _ = read_asc(out)
    ref, _ = fill_voids(zr, nodata=-9999.0)
    assert np.array_equal(_bits(f), _bits(ref.cpu().numpy()))
    r = run("fill_voids", ["--out", out, "--max-cycles", "1", "--tol", "0"])
    assert r.returncode == 0 and "warning: not converged" in r.stdout, r.stdout
    # inpaint_raster --fallback
    ck = str(tmp_path / "g.pth")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    ip = str(tmp_path / "inp.asc")
    r = run("inpaint_raster", ["--checkpoint", ck, "--out", ip, "--window", "64", "--overlap", "8"])
    assert r.returncode == 0, r.stderr
    assert " 0 holes left unfilled" not in r.stdout
    r = run("inpaint_raster", ["--checkpoint", ck, "--out", ip, "--window", "64", "--overlap", "8", "--fallback", "laplace"])
    assert r.returncode == 0, r.stderr
    assert " 0 holes left unfilled" in r.stdout and "fallback laplace:" in r.stdout
    a, _ = read_asc(ip)
    assert np.isfinite(a).all() and not (a == -9999.0).any()
    # evaluate_raster --baseline, both modes
    common = ["--block", "160", "--tile", "80", "--window", "128", "--overlap", "16"]
    js, pr, ho = (str(tmp_path / n) for n in ("r.json", "pred.asc", "holes.png"))
    r = run("evaluate_raster", ["--checkpoint", ck, "--json", js, "--pred-out", pr, "--holes-out", ho, "--baseline", "laplace",
                                "--fallback", "laplace"] + common)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("height RMSE") == 2 and "baseline laplace:" in r.stdout
    rep = json.load(open(js))
    assert rep["baseline"]["method"] == "laplace" and "fallback" in rep["inpaint"]
    js2 = str(tmp_path / "r2.json")
    r = run("evaluate_raster", ["--pred", pr, "--holes", ho, "--json", js2, "--baseline", "laplace"] + common)
    assert r.returncode == 0, r.stderr
    assert "baseline laplace:" in r.stdout
    rep2 = json.load(open(js2))
    for k in ("pixels", "height", "slope_deg", "ring", "by_area", "holes"):
        assert json.dumps(rep2["baseline"][k]) == json.dumps(rep["baseline"][k]), k
