"""GPU checks of fill_voids(solver="pcg") (csrc/voidfill.hip): conjugate gradients around the V-cycle
against the fp64 numpy oracle (tests/vfill_oracle.py) and, above its component limit, closed-form fields: max |u - u*| <=
2e-5 x range, known pixels bit for bit, bitwise determinism, convergence within the default 50 cycles with no restart, and
never more iterations than the plain solver needs cycles (max_cycles=60; running out counts as 60).

The aligned voids: the 300 x 300 void lies off the raster border, where vfill_oracle.harmonic_field is the exact fill.  The
512 x 512 left half and the 768 x 768 missing tiles touch the border, where the natural border rule makes the fill differ from
any polynomial field; there the data are vfill_pcg_mirror.border_field, which satisfies the equation with that rule exactly
(checked on the CPU against the oracle in tests/test_fill_voids_pcg_cpu.py), and the bound is the same.

Then inpaint_raster(fallback="laplace"), correct_seams, evaluate_raster(baseline="laplace") and the four CLIs with the solver."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vfill_oracle as VO
from tests import vfill_pcg_mirror as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5                        # max |u - u*| / range
MG_CYCLES = 60


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


def _check(z, mask=None, nodata=None, oracle=True, exact=None):
    """fill_voids(solver="pcg") with the default tol and max_cycles against the oracle (or the exact fp64 field `exact`); known
    pixels bit for bit; a second call bitwise equal; no more iterations than the plain solver's cycles; -> (out, info)."""
    from mvp_gan.src.fill_voids import fill_voids
    out, info = fill_voids(z, mask, nodata=nodata, solver="pcg")
    o = out.cpu().numpy()
    k = VO.known_mask(z, mask, nodata)
    assert info["unknown"] == int((~k).sum()) and info["solver"] == "pcg"
    assert np.array_equal(_bits(o[k]), _bits(z[k]))
    out2, info2 = fill_voids(z, mask, nodata=nodata, solver="pcg")
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and info2 == info
    _, mg = fill_voids(z, mask, nodata=nodata, max_cycles=MG_CYCLES)
    assert "solver" not in mg and "restarts" not in mg
    mg_cycles = mg["cycles"] if mg["converged"] else MG_CYCLES
    print("pcg", info["cycles"], "mg", mg["cycles"], mg["converged"], "change", info["change"], "tol", info["tol"])
    if not k.any():
        assert np.isnan(o).all() and info["unfilled"] == z.size and info["cycles"] == 0
        return o, info
    assert info["unfilled"] == 0 and np.isfinite(o).all()
    assert info["converged"] and info["cycles"] <= 50 and info["restarts"] == 0, info
    assert info["cycles"] <= mg_cycles, (info, mg)
    rng = float(z[k].max()) - float(z[k].min())
    if exact is not None:
        # the fp32 data differ from the field by up to half an ulp; by the maximum principle so may the fill
        data = float(np.abs(z.astype(np.float64) - exact).max())
        err = float(np.abs(o.astype(np.float64) - exact).max())
        print("err / range", err / rng, "data", data / rng)
        assert err <= BOUND * rng + data, (err, rng, info)
    elif oracle:
        err = float(np.abs(o.astype(np.float64) - VO.solve(z, k)).max())
        print("err / range", err / max(rng, 1e-30))
        assert err <= BOUND * rng + 1e-30, (err, rng, info)
    return o, info


# ---- shapes and geometries against the oracle -----------------------------------------------------------------------
def test_single_pixel_rasters(dev):
    o, info = _check(np.full((1, 1), 7.5, np.float32))
    assert info["cycles"] == 0 and info["unknown"] == 0
    _check(np.full((1, 1), np.nan, np.float32))


def test_one_level_raster_5x7(dev):
    z = _terrain(5, 7, 0)
    k = np.array([[1, 1, 1, 1, 1, 1, 1], [1, 0, 0, 0, 1, 1, 1], [1, 0, 0, 0, 0, 1, 1], [1, 1, 0, 0, 1, 1, 0],
                  [1, 1, 1, 1, 1, 0, 0]], bool)
    _check(z, k)
    _check(_terrain(16, 16, 1), ~VO.disc(16, 16, 9, 6, 5))        # the largest one-level raster


@pytest.mark.parametrize("H,W", [(1, 300), (300, 1)])
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
    _check(z, ~VO.disc(H, W, 18, 26, 9))
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


# ---- aligned voids, above the oracle's component limit --------------------------------------------------------------
@pytest.mark.parametrize("name", ["300x300 void [64:192, 128:256]", "512x512 left half", "768x768 missing tiles"])
def test_aligned_voids(dev, name):
    H, W, boxes = M.ALIGNED[name]
    if name in M.BORDER_SIDE:
        f = M.border_field(H, W, M.BORDER_SIDE[name], (150, 12, -1.5, 0.02))
    else:
        f = M.field(H, W)
    k = M.box_known(H, W, boxes)
    _check(f.astype(np.float32), k.astype(np.float32), exact=f)


def test_disc_and_missing_tile_2048(dev):
    # 2048 tiles at level 0, 8 levels: the partials of many tiles summed in tile order, most of the tiles inactive
    H = W = 2048
    f = VO.harmonic_field(H, W, (300, 40, -25, 30, 12, 3), 1024, 1024, 1024)
    k = ~VO.disc(H, W, 1300, 620, 500)
    k[512:1024, 1024:1536] = False
    _check(f.astype(np.float32), k.astype(np.float32), exact=f)


# ---- inpaint_raster, correct_seams, evaluate_raster -----------------------------------------------------------------
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
    out1, info1 = inpaint_raster(G, z, m, fallback="laplace", solver="pcg", **kw)
    o1 = out1.cpu().numpy()
    fin = np.isfinite(o0)
    assert np.array_equal(_bits(o1[fin]), _bits(o0[fin]))      # known and GAN-filled pixels bit for bit
    ref = VO.solve(o0, fin)
    rng = float(o0[fin].max()) - float(o0[fin].min())
    assert float(np.abs(o1.astype(np.float64) - ref).max()) <= BOUND * rng
    fb = info1["fallback"]
    assert info1["unfilled"] == 0 and fb["pixels"] == info0["unfilled"]
    assert fb["solver"] == "pcg" and fb["converged"] and 1 <= fb["cycles"] <= 50 and fb["restarts"] == 0
    # the default solver reports what it always did
    _, info2 = inpaint_raster(G, z, m, fallback="laplace", **kw)
    assert set(info2["fallback"]) == {"pixels", "cycles", "converged"} and fb["cycles"] <= info2["fallback"]["cycles"]


def test_correct_seams_with_both_solvers(dev):
    from mvp_gan.src.seam_correct import correct_seams
    from tg_hip import ops as O
    H, W = 257, 129
    z = _terrain(H, W, 12)
    m = np.ones((H, W), np.float32)
    m[64:192, 32:96] = 0                               # an aligned hole
    m[10:40, 100:129] = 0                              # on the raster's edge
    rng = np.random.default_rng(12)
    g = (z + 1.5 + rng.normal(0, 0.2, (H, W))).astype(np.float32)      # a fill with an offset: a step at the outlines
    a, ia = correct_seams(z, g, m, solver="mg")
    b, ib = correct_seams(z, g, m, solver="pcg")
    assert "solver" not in ia and ib["solver"] == "pcg" and ib["restarts"] == 0
    assert ia["converged"] and ib["converged"] and ib["cycles"] <= ia["cycles"]
    assert {k: ib[k] for k in ("ring", "interior", "unfilled", "order", "max_delta")} == \
        {k: ia[k] for k in ("ring", "interior", "unfilled", "order", "max_delta")}
    a, b = a.cpu().numpy(), b.cpu().numpy()
    k = m != 0
    assert np.array_equal(_bits(a[k]), _bits(z[k])) and np.array_equal(_bits(b[k]), _bits(z[k]))
    # each delta surface is within BOUND x its range of the exact one: the range of the delta raster over its known pixels
    d, _ = O.seam_delta(torch.from_numpy(z).to(dev), torch.from_numpy(m).to(dev), None, torch.from_numpy(g).to(dev), 1)
    d = d.cpu().numpy()
    drng = float(d[np.isfinite(d)].max()) - float(d[np.isfinite(d)].min())
    diff = float(np.abs(a.astype(np.float64) - b).max())
    print("seam: mg", ia["cycles"], "pcg", ib["cycles"], "diff / delta range", diff / drng)
    assert 0 < drng <= 2 * ia["max_delta"] and diff <= 2 * BOUND * drng
    b2, ib2 = correct_seams(z, g, m, solver="pcg")
    assert np.array_equal(_bits(b2.cpu().numpy()), _bits(b)) and ib2 == ib


def test_evaluate_baseline_reports_the_solver(dev, G):
    from mvp_gan.src.evaluate_raster import evaluate_raster
    H, W, c = 512, 512, 1.0
    z = _terrain(H, W, 10)
    kw = dict(cellsize=c, split="test", block=256, tile=128, seed=2, window=128, overlap=16, batch=8)
    rep0, pred0 = evaluate_raster(G, z, baseline="laplace", **kw)
    rep, pred = evaluate_raster(G, z, baseline="laplace", solver="pcg", **kw)
    assert "solver" not in rep0["baseline"]["fill"]
    fill = rep["baseline"]["fill"]
    assert fill["solver"] == "pcg" and fill["converged"] and fill["restarts"] == 0
    assert fill["cycles"] <= rep0["baseline"]["fill"]["cycles"]
    assert torch.equal(pred, pred0)
    # both fills are within BOUND x range of the exact one, so their errors differ by at most twice that
    rng = float(z.max()) - float(z.min())
    assert abs(rep["baseline"]["height"]["rmse"] - rep0["baseline"]["height"]["rmse"]) <= 2 * BOUND * rng
    json.dumps(rep)


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
    H, W, c = 256, 320, 2.0
    z = _terrain(H, W, 11)
    z[64:192, 128:256] = -9999.0                       # an aligned void, wider than a 64-px window
    dem = str(tmp_path / "dem.asc")
    _write_asc(dem, z, c, -9999)
    cwd = os.path.join(ROOT, "terra-gan_amd")
    run = lambda mod, args: subprocess.run([sys.executable, "-m", f"mvp_gan.src.{mod}", "--dem", dem] + args, cwd=cwd,
                                           capture_output=True, text=True, timeout=600, env=dict(os.environ))
    # fill_voids
    out = str(tmp_path / "filled.asc")
    r = run("fill_voids", ["--out", out, "--solver", "pcg"])
    assert r.returncode == 0, r.stderr
    assert "converged True" in r.stdout and "solver pcg" in r.stdout
    zr, _ = read_asc(dem)
    f, _ = read_asc(out)
    ref, _ = fill_voids(zr, nodata=-9999.0, solver="pcg")
    assert np.array_equal(_bits(f), _bits(ref.cpu().numpy()))
    # seam_correct on that fill plus an offset
    g = f.copy()
    g[z == -9999.0] += 2.0
    fl, sc = str(tmp_path / "fill.asc"), str(tmp_path / "seam.asc")
    _write_asc(fl, g, c)
    r = run("seam_correct", ["--filled", fl, "--out", sc, "--solver", "pcg"])
    assert r.returncode == 0, r.stderr
    assert "converged True" in r.stdout
    # inpaint_raster --fallback
    ck = str(tmp_path / "g.pth")
    torch.save({"generator_state_dict": G.state_dict()}, ck)
    ip = str(tmp_path / "inp.asc")
    r = run("inpaint_raster", ["--checkpoint", ck, "--out", ip, "--window", "64", "--overlap", "8", "--fallback", "laplace",
                               "--solver", "pcg"])
    assert r.returncode == 0, r.stderr
    assert " 0 holes left unfilled" in r.stdout and "fallback laplace:" in r.stdout and "converged True" in r.stdout
    a, _ = read_asc(ip)
    assert np.isfinite(a).all() and not (a == -9999.0).any()
    # evaluate_raster --baseline
    js = str(tmp_path / "r.json")
    r = run("evaluate_raster", ["--checkpoint", ck, "--json", js, "--baseline", "laplace", "--solver", "pcg", "--block", "128",
                                "--tile", "64", "--window", "128", "--overlap", "16"])
    assert r.returncode == 0, r.stderr
    assert "baseline laplace (solver pcg):" in r.stdout
    assert json.load(open(js))["baseline"]["fill"]["solver"] == "pcg"
