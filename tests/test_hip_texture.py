"""GPU checks of the second-difference spectrum (csrc/texture.hip, mvp_gan/src/evaluate_raster.py texture_errors,
mvp_gan/src/texture.py) against the numpy oracle of tests/texture_oracle.py.

On integer-valued rasters every second difference, square and sum is an integer below 2^53, so counts and sums are compared with
==.  On real data the counts are exact and each sum is held to 2 n 2^-53 sum|term| of the oracle's: the terms are the same
float64 numbers on both sides (nothing fused), and two summation orders of n terms differ by at most twice the classical bound
(n - 1) u sum|term| of one, u = 2^-53; n and sum|term| come from the oracle."""
import json
import math

import numpy as np
import pytest
import torch

from tests import texture_oracle as TO

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from tg_hip import lib
    lib.load()
    return torch.device("cuda:0")


def _up(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _run(dev, z, p, sel, known, octaves=5, ws=None):
    from tg_hip import ops as O
    zt, pt, st, kt = _up(dev, z, p, sel, known)
    counts, sums = O.texture_compare(zt, pt, st, kt, octaves, ws)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (10,) and sums.dtype == torch.float64 and tuple(sums.shape) == (10, 3)
    return counts.cpu().numpy(), sums.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _rects(rng, H, W, n):
    sel = np.zeros((H, W), np.uint8)
    for _ in range(n):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        sel[y:y + int(rng.integers(1, 24)), x:x + int(rng.integers(1, 40))] = 1
    return sel


def _integer_scene(H, W, seed):
    rng = np.random.default_rng(seed)
    z = rng.integers(-1000, 1001, (H, W)).astype(np.float32)
    p = rng.integers(-1000, 1001, (H, W)).astype(np.float32)
    known = (rng.random((H, W)) >= 0.03).astype(np.uint8)
    if (H, W) == (97, 130):
        sel = np.zeros((H, W), np.uint8)
        sel[27:38, 58:71] = 1                          # straddles the tile corner at (32, 64)
    elif (H, W) == (64, 192):
        sel = np.zeros((H, W), np.uint8)
        sel[3:20, 5:50] = 1                            # tile (0, 0)
        sel[40:64, 150:192] = 1                        # tile (1, 2); the four tiles in between are skipped
    elif H * W <= 9:
        sel = np.ones((H, W), np.uint8)
        known[:] = 1
    else:
        sel = _rects(rng, H, W, 4)
        sel[H - 1, W - 1] = sel[0, 0] = 1
    return z, p, sel, known


# ---- exact on integers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1, 1), (1, 40), (3, 3), (31, 63), (32, 64), (33, 65), (97, 130), (64, 192)))
def test_exact_on_integers(dev, shape):
    H, W = shape
    z, p, sel, known = _integer_scene(H, W, 100 * H + W)
    for octaves in (1, 3, 5):
        want_c, want_s, _ = TO.spectrum(z, p, sel, known, octaves)
        counts, sums = _run(dev, z, p, sel, known, octaves)
        assert counts.tolist() == want_c.tolist(), (shape, octaves)
        assert np.array_equal(sums, want_s), (shape, octaves, sums, want_s)
        assert (counts[2 * octaves:] == 0).all() and (_bits(sums[2 * octaves:]) == 0).all()
    if shape == (3, 3):
        assert counts.tolist() == [6, 2] + [0] * 8
    if shape == (1, 1):
        assert counts.tolist() == [0] * 10 and (_bits(sums) == 0).all()
    if shape == (1, 40):
        assert counts[1::2].tolist() == [0] * 5
    if shape in ((97, 130), (64, 192)):
        assert counts.min() > 0
        # the tile skip changes nothing: with one more sel pixel in every tile that had none, at a pixel that is unknown and so
        # centres no triple, every tile is staged and the bits are the same
        sel2, skipped = sel.copy(), 0
        for ty in range(0, H, 32):
            for tx in range(0, W, 64):
                if not sel[ty:ty + 32, tx:tx + 64].any():
                    ys, xs = np.nonzero(known[ty:ty + 32, tx:tx + 64] == 0)
                    if len(ys):                        # a sliver of a tile at the rim may have no unknown pixel
                        sel2[ty + ys[0], tx + xs[0]] = 1
                        skipped += 1
        assert skipped >= 4
        counts2, sums2 = _run(dev, z, p, sel2, known, 5)
        assert counts2.tolist() == counts.tolist() and np.array_equal(_bits(sums2), _bits(sums))


def test_more_workgroups_than_the_grid_cap(dev):
    """2100 tiles for 2048 workgroups: the first 52 workgroups walk two tiles each.  A raster of 3 rows keeps it small."""
    H, W = 3, 2100 * 64
    rng = np.random.default_rng(8)
    z = rng.integers(-1000, 1001, (H, W)).astype(np.float32)
    p = rng.integers(-1000, 1001, (H, W)).astype(np.float32)
    known = np.ones((H, W), np.uint8)
    sel = np.zeros((H, W), np.uint8)
    for x0 in (0, 64 * 51 + 60, 64 * 2047 + 50, 64 * 2048, 64 * 2099 + 30):
        sel[:, x0:x0 + 34] = 1
    want_c, want_s, _ = TO.spectrum(z, p, sel, known, 5)
    counts, sums = _run(dev, z, p, sel, known, 5)
    assert counts.tolist() == want_c.tolist() and np.array_equal(sums, want_s)


# ---- bounded on real data ----------------------------------------------------------------------------------------------------
def test_bounded_on_real_data(dev):
    from mvp_gan.src.evaluate_raster import texture_errors, texture_raw
    from tests.test_hip_terrain_eval import _terrain
    H, W, c, nodata = 200, 300, 2.0, -9999.0
    rng = np.random.default_rng(12)
    z = _terrain(H, W, c, 5)
    holes = np.zeros((H, W), np.uint8)
    pred = z.copy()
    for (y0, y1, x0, x1) in ((20, 70, 30, 110), (90, 130, 50, 75), (150, 200, 240, 300), (0, 12, 0, 20)):
        holes[y0:y1, x0:x1] = 1
        pred[y0:y1, x0:x1] += rng.normal(0, 0.3, (y1 - y0, x1 - x0)).astype(np.float32)
    pred[33, 44] = np.nan                              # a pixel the fill left
    z[19, 60] = np.nan                                 # next to a hole: an arm of the row below
    z[100, 49] = nodata                                # next to a hole
    z[160, 250] = nodata                               # inside a hole: not scored, and no arm
    mask = np.ones((H, W), np.float32)
    mask[60:75, 100:140] = 0                           # cuts a corner off the first hole
    known = np.isfinite(z) & (z != np.float32(nodata)) & (mask != 0) & np.isfinite(pred)
    want_c, want_s, want_abs = TO.spectrum(z, pred, holes, known, 5)
    counts, sums = texture_raw(z, pred, holes, cellsize=c, mask=mask, nodata=nodata)
    assert counts == want_c.tolist() and min(counts) > 1000
    sums = np.array(sums)
    assert np.isfinite(sums).all() and np.isfinite(want_s).all()
    for s in range(10):
        for q, name in enumerate(("Szz", "Spp", "Szp")):
            err, bound = abs(sums[s, q] - want_s[s, q]), 2.0 * want_c[s] * U * want_abs[s, q]
            print(f"scale {s} {name}: got {sums[s, q]:.17g} ref {want_s[s, q]:.17g} rel diff {err / abs(want_s[s, q]):.3e} "
                  f"bound rel {bound / abs(want_s[s, q]):.3e}")
            assert err <= bound, (s, name, sums[s, q], want_s[s, q], bound)
    # the same relief around zero, in millimetres of a metre: at 200 m every float32 is a multiple of 2^-16 and the squares above
    # add up without a rounding in float64; here the exponents vary and the sums round, so the order of the additions shows
    zs, ps = ((a - np.float32(200)) * np.float32(1e-3) for a in (z, pred))
    zs[z == np.float32(nodata)] = nodata
    want_c2, want_s2, want_abs2 = TO.spectrum(zs, ps, holes, known, 5)
    counts2, sums2 = texture_raw(zs, ps, holes, cellsize=c, mask=mask, nodata=nodata)
    assert counts2 == counts == want_c2.tolist()
    worst = 0.0
    for s in range(10):
        for q in range(3):
            err, bound = abs(sums2[s][q] - want_s2[s, q]), 2.0 * want_c2[s] * U * want_abs2[s, q]
            worst = max(worst, err / bound)
            assert err <= bound, (s, q, sums2[s][q], want_s2[s, q], bound)
    print("small relief: worst |diff| / bound", worst, "sums that differ from numpy's", int((np.array(sums2) != want_s2).sum()), "of 30")
    d = texture_errors(z, pred, holes, cellsize=c, mask=mask, nodata=nodata)
    assert d["octaves"] == 5 and d["scales_scored"] == 10 and [s["triples"] for s in d["scales"]] == counts
    assert all(s["ratio"] > 1.0 and 0 < s["corr"] < 1 for s in d["scales"][:2])      # the noise roughens the shortest lag
    assert json.loads(json.dumps(d)) == d


# ---- the analytic cases through texture_errors -----------------------------------------------------------------------------
def _plane(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (3 * x - 2 * y + 7).astype(np.float32)


def _analytic():
    H, W = 80, 90
    z = _plane(H, W)
    x = np.arange(W, dtype=np.float32)[None, :]
    hole = np.zeros((H, W), np.uint8)
    hole[20:60, 20:70] = 1
    yield "quadratic", z, z + 2 * x * x, hole
    y, x = np.mgrid[0:H, 0:W]
    yield "checkerboard", z, (z + 3.0 * (1 - 2 * ((x + y) & 1))).astype(np.float32), np.ones((H, W), np.uint8)
    r = np.random.default_rng(3).integers(-1000, 1001, (H, W)).astype(np.float32)
    yield "identity", r, r.copy(), hole


@pytest.mark.parametrize("case", list(_analytic()), ids=lambda c: c[0])
def test_analytic_cases(dev, case):
    from mvp_gan.src.evaluate_raster import assemble_texture, texture_errors
    name, z, p, hole = case
    for octaves, c in ((5, 1.0), (2, 2.5)):
        counts, sums, _ = TO.spectrum(z, p, hole, np.ones_like(hole), octaves)
        want = assemble_texture(counts.tolist(), sums.tolist(), cellsize=c, octaves=octaves)
        got = texture_errors(z, p, hole, cellsize=c, octaves=octaves)
        assert got == want and json.dumps(got) == json.dumps(want), (name, got, want)
    got = texture_errors(z, p, hole, cellsize=1.0)
    if name == "quadratic":
        assert [s["fill_rms"] for s in got["scales"][1::2]] == [4.0 * h * h for h in (1, 2, 4, 8, 16)]
        assert [s["fill_rms"] for s in got["scales"][0::2]] == [(8.0 * h ** 4) ** 0.5 for h in (1, 2, 4, 8, 16)]
    if name == "checkerboard":
        assert [s["fill_rms"] for s in got["scales"]] == [12.0] + [0.0] * 9
    if name == "identity":
        assert all(s["ratio"] == 1.0 and s["corr"] == 1.0 for s in got["scales"]) and got["log_ratio_rms"] == 0.0


# ---- determinism -------------------------------------------------------------------------------------------------------------
def test_determinism_and_workspace(dev):
    from tg_hip import ops as O
    from tests.test_hip_terrain_eval import _terrain
    H, W = 200, 300
    rng = np.random.default_rng(2)
    z = _terrain(H, W, 1.0, 3)
    p = (z + rng.normal(0, 0.5, (H, W))).astype(np.float32)
    sel = _rects(rng, H, W, 6)
    known = (rng.random((H, W)) >= 0.02).astype(np.uint8)
    a = _run(dev, z, p, sel, known)
    b = _run(dev, z, p, sel, known)
    ws = O.texture_ws(H, W)
    assert ws.dtype == torch.uint8 and ws.is_cuda and ws.numel() == 7 * 5 * 240
    ws.fill_(0xFF)
    c = _run(dev, z, p, sel, known, ws=ws)
    big = torch.full((ws.numel() + 4096,), 0xFF, dtype=torch.uint8, device=dev)
    d = _run(dev, z, p, sel, known, ws=big)
    for other in (b, c, d):
        assert a[0].tolist() == other[0].tolist() and np.array_equal(_bits(a[1]), _bits(other[1]))
    assert a[0].min() > 0 and np.isfinite(a[1]).all()


# ---- one surface -------------------------------------------------------------------------------------------------------------
def test_texture_spectrum(dev, tmp_path, capsys):
    from mvp_gan.src.asc import write_asc
    from mvp_gan.src.texture import main, texture_spectrum
    from tests.test_hip_terrain_eval import _terrain
    H, W, c, nodata = 90, 140, 2.0, -9999.0
    z = _terrain(H, W, c, 11)
    z[10:14, 20:30] = nodata
    z[50, 60] = np.nan
    mask = np.ones((H, W), np.uint8)
    mask[70:, :15] = 0
    known = np.isfinite(z) & (z != np.float32(nodata)) & (mask != 0)

    def check(d, sel, octaves):
        counts, sums, asum = TO.spectrum(z, z, sel, known, octaves)
        assert d["octaves"] == octaves and len(d["scales"]) == 2 * octaves
        for s, e in enumerate(d["scales"]):
            h = 1 << (s // 2)
            assert list(e) == ["lag_px", "class", "lag_m", "triples", "rms"]
            assert (e["lag_px"], e["class"], e["triples"]) == (h, ("axial", "diagonal")[s % 2], counts[s])
            assert e["lag_m"] == h * c * (math.sqrt(2.0) if s % 2 else 1.0)
            ref = (sums[s, 0] / counts[s]) ** 0.5
            assert abs(e["rms"] - ref) <= 2.0 * counts[s] * U * ref       # sqrt halves the relative bound of the sum
        assert json.loads(json.dumps(d)) == d

    check(texture_spectrum(z, mask, nodata=nodata, cellsize=c), np.ones((H, W), np.uint8), 5)
    where = np.zeros((H, W), np.float32)
    where[30:60, 40:100] = 2.5                         # nonzero = counts
    d = texture_spectrum(z, mask, nodata=nodata, cellsize=c, octaves=3, where=where)
    check(d, where, 3)
    assert d["scales"][0]["triples"] == 2 * (30 * 60 - 3)      # per step, the NaN at (50, 60) centres one triple and is an arm of two
    assert texture_spectrum(np.zeros((1, 1), np.float32)) == {"octaves": 5, "scales": [
        {"lag_px": 1 << (s // 2), "class": ("axial", "diagonal")[s % 2], "lag_m": (1 << (s // 2)) * (math.sqrt(2.0) if s % 2 else 1.0),
         "triples": 0, "rms": None} for s in range(10)]}
    # the CLI on a small grid
    hdr = [("ncols", str(W)), ("nrows", str(H)), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", "2"), ("NODATA_value", "-9999")]
    write_asc(tmp_path / "in.asc", z, hdr)
    capsys.readouterr()
    got = main(["--dem", str(tmp_path / "in.asc"), "--octaves", "2", "--json", str(tmp_path / "t.json")])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 4 and out[0].startswith("lag  1 px axial") and "triples" in out[3]
    assert json.load(open(tmp_path / "t.json")) == got == texture_spectrum(z, nodata=nodata, cellsize=2.0, octaves=2)


# ---- evaluate_raster ---------------------------------------------------------------------------------------------------------
def test_evaluate_raster_texture(dev, tmp_path, capsys):
    """End to end on the scene of test_evaluate_raster_wetness: the GAN, the harmonic baseline and the IDW fill, each with its
    texture entry; without the option the report is what it was.  No ranking of the fills is asserted: the generator is seeded
    and untrained."""
    from mvp_gan.src.asc import write_asc, write_mask
    from mvp_gan.src.evaluate_raster import eval_holes, evaluate_raster, main, texture_errors, texture_summary
    from mvp_gan.src.models import PConvUNet
    from tests.test_hip_terrain_eval import _terrain
    torch.manual_seed(7)
    G = PConvUNet().to(dev)
    H, W, c = 400, 520, 2.0
    z = _terrain(H, W, c, 8)
    kw = dict(cellsize=c, block=160, tile=80, window=128, overlap=16, baseline="laplace", compare=("idw",))
    rep, pred = evaluate_raster(G, z, texture=True, texture_octaves=4, **kw)
    plain, pred0 = evaluate_raster(G, z, **kw)                                # the report of the code as it stood
    assert torch.equal(pred, pred0)

    def strip(r):
        return {k: (strip(v) if isinstance(v, dict) and k in ("baseline", "compare", "idw") else v) for k, v in r.items()
                if k != "texture"}
    assert "texture" not in plain and "texture" not in plain["baseline"] and "texture" not in plain["compare"]["idw"]
    assert json.dumps(strip(rep)) == json.dumps(plain) and set(rep) - set(plain) == {"texture"}
    for d in (rep["texture"], rep["baseline"]["texture"], rep["compare"]["idw"]["texture"]):
        assert list(d) == ["octaves", "scales", "scales_scored", "log_ratio_rms"] and d["octaves"] == 4 and len(d["scales"]) == 8
        assert d["scales_scored"] == 8 and all(s["triples"] > 0 and s["truth_rms"] > 0 for s in d["scales"])
        assert texture_summary(d).startswith("texture: second differences fill / truth, 1 px axial ratio")
        json.dumps(d)
    zt = torch.from_numpy(z).to(dev)
    hm, keep, _ = eval_holes(zt, None, split="test", block=160, tile=80, cellsize=c)
    assert json.dumps(rep["texture"]) == json.dumps(texture_errors(zt, pred, hm, cellsize=c, octaves=4))
    # scoring mode
    hdr = [("ncols", str(W)), ("nrows", str(H)), ("xllcorner", "0"), ("yllcorner", "0"), ("cellsize", "2"), ("NODATA_value", "-9999")]
    write_asc(tmp_path / "dem.asc", z, hdr)
    write_asc(tmp_path / "pred.asc", pred.cpu().numpy(), hdr)
    write_mask(tmp_path / "holes.asc", hm.cpu().numpy(), hdr)
    capsys.readouterr()
    args = ["--dem", str(tmp_path / "dem.asc"), "--pred", str(tmp_path / "pred.asc"), "--holes", str(tmp_path / "holes.asc")]
    r2 = main(args + ["--texture", "--octaves", "4", "--baseline", "laplace"])
    out = capsys.readouterr().out.splitlines()
    assert json.dumps(r2["texture"]) == json.dumps(rep["texture"])          # the .asc files hold every float32 bit
    assert texture_summary(r2["texture"]) in out and f"baseline laplace {texture_summary(r2['baseline']['texture'])}" in out
    r3 = main(args)
    assert "texture" not in r3 and not any("texture" in line for line in capsys.readouterr().out.splitlines())


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_before_any_launch(dev):
    from mvp_gan.src.evaluate_raster import evaluate_raster, texture_errors
    from mvp_gan.src.texture import texture_spectrum
    from tg_hip import ops as O
    z = np.zeros((20, 30), np.float32)
    for bad in (0, 6, 1.5, True):
        with pytest.raises(ValueError, match="octaves"):
            texture_errors(z, z, z, cellsize=1.0, octaves=bad)
        with pytest.raises(ValueError, match="octaves"):
            texture_spectrum(z, octaves=bad)
        with pytest.raises(ValueError, match="octaves"):
            evaluate_raster(None, np.zeros((400, 400), np.float32), cellsize=1.0, block=160, tile=80, texture=True, texture_octaves=bad)
    assert texture_errors(z, z, np.ones_like(z), cellsize=1.0, octaves=np.int64(2))["octaves"] == 2
    with pytest.raises(ValueError, match="pred"):
        texture_errors(z, np.zeros((20, 31), np.float32), z, cellsize=1.0)
    with pytest.raises(ValueError, match="holes"):
        texture_errors(z, z, np.zeros((21, 30), np.uint8), cellsize=1.0)
    zt = torch.zeros(20, 30, device=dev)
    u8 = torch.ones(20, 30, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="z must be"):
        O.texture_compare(zt.double(), zt, u8, u8)
    with pytest.raises(ValueError, match="p must be"):
        O.texture_compare(zt, zt.cpu(), u8, u8)
    with pytest.raises(ValueError, match="sel must be"):
        O.texture_compare(zt, zt, u8.float(), u8)
    with pytest.raises(ValueError, match="known must be"):
        O.texture_compare(zt, zt, u8, u8[:, :29])
    with pytest.raises(ValueError, match="known must be"):
        O.texture_compare(zt, zt, u8, u8.t().contiguous().t())
    for bad in (0, 6, 1.5, True):
        with pytest.raises(ValueError, match="octaves"):
            O.texture_compare(zt, zt, u8, u8, bad)
    ws = O.texture_ws(20, 30, dev)
    with pytest.raises(ValueError, match="ws must be"):
        O.texture_compare(zt, zt, u8, u8, 5, ws[:ws.numel() - 1])
    with pytest.raises(ValueError, match="ws must be"):
        O.texture_compare(zt, zt, u8, u8, 5, ws.cpu())
    with pytest.raises(ValueError):
        O.texture_ws(0, 5)
    counts, sums = O.texture_compare(zt, zt, u8, u8, 5, ws)                 # and the accepted call: a flat raster
    assert counts.cpu().tolist() == TO.spectrum(z, z, np.ones_like(z), np.ones_like(z))[0].tolist() and (sums == 0).all()
