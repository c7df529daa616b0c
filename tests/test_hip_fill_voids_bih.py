"""GPU checks of fill_voids(method="biharmonic") (csrc/voidfill.hip).

Closed form: tests/vfill_bih_oracle.bih_poly satisfies D(D(f)) = 0 off the raster border, so on voids at least 2 pixels from
it the fill must return it: max |u - f| <= 2e-5 x range (the bound of the harmonic fill, section 8n), while the harmonic fill
of the same scene misses it by more than 1e-2 x range.  Small scenes: the dense fp64 normal equations of the same module, same
bound.  Everywhere: known pixels bit for bit, a second call bitwise equal with equal info, no restarts, and convergence within
the numpy mirror's own iteration count (tests/vfill_bih_mirror.py, MIRROR_ITERATIONS below and in section 8q) plus 25 %, rounded
up: fused multiply-adds in the fp32 cycle move a count by one or two.  Then `inner`, evaluate_raster(baseline="biharmonic")
and the CLI."""
import math

import numpy as np
import pytest
import torch

from tests import vfill_bih_mirror as BM
from tests import vfill_bih_oracle as BO
from tests import vfill_oracle as VO

pytestmark = pytest.mark.gpu
BOUND = 2e-5                        # max |u - u*| / range of z over K
HARMONIC_MISS = 1e-2                # the harmonic fill is further than this from bih_poly

# outer iterations of the mirror with the kernels' storage types, inner = 3 (tests/test_fill_voids_bih_cpu.py holds it to them)
MIRROR_ITERATIONS = {
    "37x53 disc, cubic": 13,
    "128x160 void [30:93, 61:130], cubic": 26,
    "300x300 void [64:192, 128:256], cubic": 38,
    "5x7 hole": 7,
    "16x16 hole": 8,
    "32x64 disc": 14,
    "33x65 corner past the tile": 13,
    "70x140 four-tile corner": 11,
    "40x130 ring in a tile without unknowns": 8,
    "48x80 edges and a corner": 14,
    "96x80 left half": 30,
    "1x300 runs": 32,
    "300x1 runs": 31,
    "12x9 one known": 1,
    "40x50 nan inf nodata mask": 11,
    "48x64 3% known": 40,
}
CUBIC = [n for n in MIRROR_ITERATIONS if n.endswith("cubic")]
INNER_SCENE = "128x160 void [30:93, 61:130]"             # the unaligned scene, section 8q's smooth terrain
ALIGNED_SCENE = "300x300 void [64:192, 128:256]"


def budget(name):
    return math.ceil(1.25 * MIRROR_ITERATIONS[name])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _fill(z, mask=None, nodata=None, **kw):
    """fill_voids(method="biharmonic"): known pixels bit for bit, a second call bitwise equal with equal info, info keys."""
    from mvp_gan.src.fill_voids import fill_voids
    out, info = fill_voids(z, mask, nodata=nodata, method="biharmonic", **kw)
    o = out.cpu().numpy()
    k = VO.known_mask(z, mask, nodata)
    assert info["unknown"] == int((~k).sum()) and info["method"] == "biharmonic" and info["inner"] == kw.get("inner", 3)
    assert "solver" not in info
    assert np.array_equal(_bits(o[k]), _bits(z[k]))
    out2, info2 = fill_voids(z, mask, nodata=nodata, method="biharmonic", **kw)
    assert np.array_equal(_bits(out2.cpu().numpy()), _bits(o)) and info2 == info
    assert info["vcycles"] == 2 * info["inner"] * (info["cycles"] + 1) or info["cycles"] == 0
    print("iterations", info["cycles"], "vcycles", info["vcycles"], "change", info["change"], "tol", info["tol"])
    return o, info, k


@pytest.mark.parametrize("name", CUBIC)
def test_reproduces_the_cubic_the_harmonic_fill_misses(dev, name):
    from mvp_gan.src.fill_voids import fill_voids
    z, known = BM.case(name)
    H, W = z.shape
    ys, xs = np.nonzero(~known)
    assert ys.min() >= 2 and xs.min() >= 2 and ys.max() < H - 2 and xs.max() < W - 2
    exact = BO.bih_poly_raster(H, W)
    o, info, k = _fill(z, known.astype(np.float32), max_cycles=budget(name))
    rng = float(z[k].max()) - float(z[k].min())
    err = float(np.abs(o.astype(np.float64) - exact).max())
    print(name, "err / range", err / rng, "mirror", MIRROR_ITERATIONS[name])
    assert info["converged"] and info["restarts"] == 0 and info["unfilled"] == 0, info
    assert err <= BOUND * rng, (err / rng, info)
    h, hinfo = fill_voids(z, known.astype(np.float32), solver="pcg")
    miss = float(np.abs(h.cpu().numpy().astype(np.float64) - exact).max())
    print("harmonic miss / range", miss / rng)
    assert hinfo["converged"] and "method" not in hinfo and "vcycles" not in hinfo and "inner" not in hinfo
    assert miss > HARMONIC_MISS * rng


@pytest.fixture(scope="module")
def oracle():
    """name -> the dense fp64 fill, computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            z, m, nd = BM.small_scene(name)
            k = VO.known_mask(z, m, nd)
            # one known pixel: the range is 0 and the fill is that value exactly, which the dense solve only rounds to
            cache[name] = np.full(z.shape, float(z[3, 4])) if name == "12x9 one known" else BO.solve(np.where(k, z, 0), k)
            cache[name].setflags(write=False)
        return cache[name]
    return get


@pytest.mark.parametrize("name", [n for n in BM.SMALL_SCENES if n in MIRROR_ITERATIONS])
def test_against_the_dense_oracle(dev, oracle, name):
    z, m, nd = BM.small_scene(name)
    assert int((~VO.known_mask(z, m, nd)).sum()) <= BO.MAX_UNKNOWN
    o, info, k = _fill(z, m, nd, max_cycles=budget(name))
    rng = float(z[k].max()) - float(z[k].min())
    err = float(np.abs(o.astype(np.float64) - oracle(name)).max())
    print(name, "err / range", err / max(rng, 1e-30), "mirror", MIRROR_ITERATIONS[name])
    assert info["converged"] and info["restarts"] == 0 and info["unfilled"] == 0 and np.isfinite(o).all(), info
    assert err <= BOUND * rng, (err, rng, info)
    if name == "12x9 one known":
        assert np.array_equal(o, np.full(z.shape, z[3, 4])) and info["change"] == 0.0


def test_all_known_and_nothing_known(dev):
    for name in ("1x1 all known", "20x30 all known"):
        z, m, nd = BM.small_scene(name)
        o, info, _ = _fill(z, m, nd)
        assert np.array_equal(_bits(o), _bits(z)) and info["cycles"] == 0 and info["vcycles"] == 0 and info["converged"]
        assert info["unknown"] == 0 and info["unfilled"] == 0 and info["restarts"] == 0
    z, m, nd = BM.small_scene("20x30 nothing known")
    o, info, _ = _fill(z, m, nd)
    assert np.isnan(o).all() and info["unfilled"] == z.size == info["unknown"] and info["cycles"] == 0
    assert not info["converged"]
    z1 = np.full((1, 1), np.nan, np.float32)
    o, info, _ = _fill(z1)
    assert np.isnan(o).all() and info["unfilled"] == 1


def test_inner_1_and_5_reach_the_same_fill(dev):
    z, known = BM.case(INNER_SCENE)
    m = known.astype(np.float32)
    rng = float(z[known].max()) - float(z[known].min())
    o1, i1, _ = _fill(z, m, inner=1)
    o5, i5, _ = _fill(z, m, inner=5)
    print("inner 1:", i1["cycles"], "inner 5:", i5["cycles"])
    assert i1["converged"] and i5["converged"] and i1["restarts"] == 0 and i5["restarts"] == 0
    assert i1["vcycles"] == 2 * (i1["cycles"] + 1) and i5["vcycles"] == 10 * (i5["cycles"] + 1)
    assert float(np.abs(o1.astype(np.float64) - o5).max()) <= 2 * BOUND * rng


def test_inner_1_does_not_converge_on_the_aligned_void(dev):
    # a property of the bare cycle on tile-aligned voids (section 8n), found by the mirror too: not a fault
    z, known = BM.case(ALIGNED_SCENE)
    o, info, _ = _fill(z, known.astype(np.float32), inner=1, max_cycles=100)
    assert not info["converged"] and info["cycles"] == 100, info
    assert np.isfinite(o).all()


def test_evaluate_raster_baseline(dev):
    from mvp_gan.src.evaluate_raster import BASELINES, baseline_report, eval_holes, terrain_errors
    from mvp_gan.src.fill_voids import fill_voids
    assert "biharmonic" in BASELINES
    z = torch.from_numpy(BM.terrain(192, 256, 9)).to(dev)
    hm, keep, _ = eval_holes(z, split="test")
    rep = baseline_report(z, hm, keep, cellsize=1.0, method="biharmonic")
    fill, finfo = fill_voids(z, keep, method="biharmonic")
    want = terrain_errors(z, fill, hm, keep, cellsize=1.0)
    assert rep["method"] == "biharmonic" and rep["fill"] == finfo and finfo["converged"]
    for key in want:
        assert rep[key] == want[key], key


def test_evaluate_raster_passes_the_baseline_through(dev):
    from mvp_gan.src.evaluate_raster import baseline_report, eval_holes, evaluate_raster
    from mvp_gan.src.models import PConvUNet
    torch.manual_seed(11)
    G = PConvUNet().to(dev)
    z = torch.from_numpy(BM.terrain(192, 256, 9)).to(dev)
    rep, _ = evaluate_raster(G, z, cellsize=1.0, baseline="biharmonic")
    hm, keep, _ = eval_holes(z, split="test")
    want = baseline_report(z, hm, keep, cellsize=1.0, method="biharmonic")
    assert rep["baseline"]["method"] == "biharmonic" and rep["baseline"]["fill"]["method"] == "biharmonic"
    assert rep["baseline"]["height"] == want["height"] and rep["baseline"]["fill"] == want["fill"]


def test_cli_round_trips_an_asc(dev, tmp_path):
    from mvp_gan.src import fill_voids as FV
    from mvp_gan.src.asc import read_asc, write_asc
    z, known = BM.case("37x53 disc, cubic")
    holed = np.where(known, z, np.float32(-9999.0))
    header = [("ncols", "53"), ("nrows", "37"), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", "1"),
              ("NODATA_value", "-9999")]
    src, dst = str(tmp_path / "in.asc"), str(tmp_path / "out.asc")
    write_asc(src, holed, header)
    info = FV.main(["--dem", src, "--out", dst, "--method", "biharmonic", "--inner", "2"])
    assert info["method"] == "biharmonic" and info["inner"] == 2 and info["converged"] and info["cycles"] <= 200
    got, _ = read_asc(dst)
    back, _ = read_asc(src)
    k = back != -9999.0
    want, winfo = FV.fill_voids(back, nodata=-9999.0, method="biharmonic", inner=2)
    assert winfo == info
    w = want.cpu().numpy()
    assert np.array_equal(got[k], back[k])
    rng = float(back[k].max() - back[k].min())
    assert np.abs(got.astype(np.float64) - w).max() <= 1e-5 * rng          # the .asc's decimal digits
    assert np.abs(got.astype(np.float64) - BO.bih_poly_raster(37, 53)).max() <= BOUND * rng + 1e-5 * rng
