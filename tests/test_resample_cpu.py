"""Host-side checks of the raster resampling (mvp_gan/src/resample.py) that need no GPU: the scale, the
plan and its integer weights against the Fraction geometry of tests/resample_oracle.py, properties of the oracle itself, the
validation of every new argument and CLI flag, and the .asc header arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

from tests import resample_oracle as XO

SCALES_DOWN = [(2, 1), (3, 1), (5, 2), (10, 3), (16, 1), (1, 1)]
SCALES_UP = [(1, 2), (2, 3), (3, 10), (1, 4)]


# ---- scale ----------------------------------------------------------------------------------------------------------
def test_resample_scale_accepts():
    from mvp_gan.src.resample import resample_scale
    for c, t, want in [(0.25, 1, Fraction(4)), (0.5, 1, Fraction(2)), (2, 1, Fraction(1, 2)), (0.3, 1, Fraction(10, 3)),
                       (1.5, 1, Fraction(2, 3)), (1, 1, Fraction(1)), (1.0, 16.0, Fraction(16)), (4, 1, Fraction(1, 4))]:
        got = resample_scale(c, t)
        assert isinstance(got, Fraction) and got == want == XO.scale(c, t), (c, t, got)


def test_resample_scale_rejects():
    from mvp_gan.src.resample import resample_scale
    for c, t in [(1, 0.2), (20, 1), (1, 2 ** 0.5), (1, 16.5), (0, 1), (1, 0), (-1, 1), (1, float("nan")), (float("inf"), 1)]:
        with pytest.raises(ValueError, match="resample"):
            resample_scale(c, t)


def test_resample_scale_1e6_rule():
    from mvp_gan.src.resample import resample_scale
    assert resample_scale(1.0, 2.0 * (1 + 5e-7)) == 2                 # within 1e-6 relative of 2/1
    with pytest.raises(ValueError, match="no fraction"):
        resample_scale(1.0, 2.0 * (1 + 2e-5))                         # the nearest q <= 64 fraction is further away than that
    assert resample_scale(3.0, 10.0 + 5e-6) == Fraction(10, 3)
    with pytest.raises(ValueError, match="no fraction"):
        resample_scale(1.0, 1.0 + 1.0 / 200)                          # 201/200: denominator above 64


def test_coverage_fraction():
    from mvp_gan.src.resample import coverage_fraction
    assert coverage_fraction(0.5) == (1, 2) and coverage_fraction(1) == (1, 1) and coverage_fraction(1 / 3) == (1, 3)
    assert coverage_fraction(0.001) == (1, 1000)
    for bad in (0, -0.1, 1.0001, float("nan"), None, "0.5", True, 1e-5):
        with pytest.raises(ValueError, match="min_coverage"):
            coverage_fraction(bad)


# ---- plan -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p,q", SCALES_DOWN + SCALES_UP)
def test_plan_sizes(p, q):
    from mvp_gan.src.resample import resample_plan
    for H, W in [(203, 317), (257, 130), (40, 41), (1, 7)]:
        pl = resample_plan(H, W, p, q)
        assert (pl.Ho, pl.Wo) == (-(-H * q // p), -(-W * q // p)) == (XO.out_size(H, p, q), XO.out_size(W, p, q))
        assert len(pl.rows) == pl.Ho and len(pl.cols) == pl.Wo and (pl.p, pl.q) == (p, q)
        # the grid covers the raster, and its last pixel starts inside it
        assert pl.Ho * p >= H * q > (pl.Ho - 1) * p and pl.Wo * p >= W * q > (pl.Wo - 1) * p


def test_plan_rejects():
    from mvp_gan.src.resample import resample_plan
    for args in [(0, 5, 2, 1), (5, 0, 2, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 17, 1), (5, 5, 1, 5), (5, 5, 130, 65)]:
        with pytest.raises(ValueError, match="resample_plan"):
            resample_plan(*args)


@pytest.mark.parametrize("p,q", SCALES_DOWN)
@pytest.mark.parametrize("N", [203, 317, 130, 41])
def test_area_weights(p, q, N):
    """Every footprint's weights sum to its clipped length, p except at the clipped last pixel; every source pixel's weights
    sum to q, its own length in units of 1/q pixel, over the outputs it touches (in two dimensions: footprint area up to
    p * p, and q * q per source pixel).  The taps and weights are those of the Fraction geometry."""
    from mvp_gan.src.resample import area_axis
    ax = area_axis(N, p, q)
    ref = XO.area_axis(N, p, q)
    per_source = np.zeros(N, np.int64)
    for I, (t, (i0, w)) in enumerate(zip(ax, ref)):
        assert t.start == i0 and [Fraction(v, q) for v in t.weights] == w and all(v > 0 for v in t.weights)
        clipped = min((I + 1) * p, N * q) - I * p
        assert sum(t.weights) == clipped and (clipped == p or I == len(ax) - 1)
        assert 0 <= t.start and t.start + len(t.weights) <= N
        per_source[t.start:t.start + len(t.weights)] += t.weights
    assert (per_source == q).all()
    last = ax[-1]
    assert sum(last.weights) == N * q - (len(ax) - 1) * p and last.start + len(last.weights) == N


@pytest.mark.parametrize("p,q", SCALES_UP)
@pytest.mark.parametrize("N", [203, 130, 41])
def test_interp_weights(p, q, N):
    from mvp_gan.src.resample import interp_axis
    ax = interp_axis(N, p, q)
    ref = XO.interp_axis(N, p, q)
    m = 2 * q
    for t, (taps, cubic, lin, pos) in zip(ax, ref):
        assert list(t.taps) == taps and t.centre == pos
        assert sum(t.cubic) == 2 * m ** 3 and [Fraction(v, 2 * m ** 3) for v in t.cubic] == cubic
        assert sum(t.linear) == m and [Fraction(v, m) for v in t.linear] == lin
        assert all(abs(v) < 2 ** 23 for v in t.cubic)                # exact in fp32
        assert t.linear[t.centre - 1] > 0                             # the containing pixel always carries weight
        assert all(0 <= i < N for i in t.taps)


# ---- properties of the oracle ---------------------------------------------------------------------------------------
def _plane(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 900.0 + 0.25 * x - 0.125 * y                                  # exact in fp32
    assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
    return z.astype(np.float32)


@pytest.mark.parametrize("p", [1, 2, 3, 16])
def test_oracle_area_reproduces_a_plane_at_integer_scales(p):
    """An integer scale's footprints are whole pixels, whose centroid is the output centre.  (At a fractional scale a pixel cut
    by the footprint still counts at its own centre, so the mean of a plane is its value at the weighted mean of the tap
    centres, which the next test checks.)"""
    H, W = 83, 131
    r = XO.area(_plane(H, W), p=p, q=1)
    Ho, Wo = H // p, W // p                                           # away from the clipped edge
    Y, X = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    want = 900.0 + 0.25 * ((X + 0.5) * p - 0.5) - 0.125 * ((Y + 0.5) * p - 0.5)
    assert r["known"].all() and np.abs(r["value"][:Ho, :Wo] - want).max() <= 1e-9
    assert (r["n"][:Ho, :Wo] == p * p).all()


@pytest.mark.parametrize("p,q", [(5, 2), (10, 3)])
def test_oracle_area_of_a_plane_at_fractional_scales(p, q):
    from mvp_gan.src.resample import area_axis
    H, W = 83, 131
    r = XO.area(_plane(H, W), p=p, q=q)
    cen = lambda ax: np.array([sum(w * (t.start + k) for k, w in enumerate(t.weights)) / sum(t.weights) for t in ax])
    cy, cx = cen(area_axis(H, p, q)), cen(area_axis(W, p, q))
    want = 900.0 + 0.25 * cx[None, :] - 0.125 * cy[:, None]
    assert r["known"].all() and np.abs(r["value"] - want).max() <= 1e-9


@pytest.mark.parametrize("p,q", SCALES_UP)
def test_oracle_interp_reproduces_a_plane(p, q):
    H, W = 47, 61
    r = XO.interp(_plane(H, W), p=p, q=q)
    Ho, Wo = r["value"].shape
    Y, X = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    cy, cx = ((2 * Y + 1) * p - q) / (2 * q), ((2 * X + 1) * p - q) / (2 * q)
    inner = (cy >= 1) & (cy <= H - 3) & (cx >= 1) & (cx <= W - 3)     # away from the clamped border
    want = 900.0 + 0.25 * cx - 0.125 * cy
    assert r["known"].all() and inner.any() and (r["n"] == 16).all()
    assert np.abs(r["value"] - want)[inner].max() <= 1e-9
    # bilinear (a hole next to every pixel that kills the 16-tap stencil, not the 4-tap one) reproduces it too
    m = np.ones((H, W), np.float32)
    m[::7, ::7] = 0
    r = XO.interp(_plane(H, W), m, p=p, q=q)
    sel = inner & r["known"] & (r["n"] == 4) & (r["R"] > 0)
    k = XO.known(_plane(H, W), m)
    four = np.ones_like(sel)
    for dy in (0, 1):
        for dx in (0, 1):
            four &= k[np.clip(np.floor(cy).astype(int) + dy, 0, H - 1), np.clip(np.floor(cx).astype(int) + dx, 0, W - 1)]
    sel &= four
    assert sel.any() and np.abs(r["value"] - want)[sel].max() <= 1e-9


def test_oracle_preserves_constants_exactly_and_scale_1_is_the_identity():
    rng = np.random.default_rng(0)
    H, W = 45, 67
    c = np.float32(912.34564)
    z = np.full((H, W), c, np.float32)
    m = (rng.random((H, W)) > 0.3).astype(np.float32)
    for p, q in SCALES_DOWN:
        r = XO.area(z, m, p=p, q=q, cov=Fraction(1, 1000))
        assert r["known"].any() and (r["value"][r["known"]] == np.float64(c)).all() and np.isnan(r["value"][~r["known"]]).all()
    for p, q in SCALES_UP:
        r = XO.interp(z, m, p=p, q=q)
        assert r["known"].any() and (r["value"][r["known"]] == np.float64(c)).all()
    z = (900 + 50 * rng.random((H, W))).astype(np.float32)
    z[3, 4] = np.nan
    z[5, 6] = -9999.0
    r = XO.area(z, m, -9999.0, p=1, q=1)
    k = XO.known(z, m, -9999.0)
    assert np.array_equal(r["known"], k) and np.array_equal(r["value"][k], z[k].astype(np.float64))
    assert np.isnan(r["value"][~k]).all() and not k[3, 4] and not k[5, 6]


def test_oracle_coverage_is_exact_at_a_tie():
    z = np.full((4, 4), 900.0, np.float32)
    m = np.ones((4, 4), np.float32)
    m[0:2, 0] = 0                                                     # half of output (0, 0) at scale 2
    m[0:2, 2] = 0
    m[0, 3] = 0                                                       # three quarters of output (0, 1)
    r = XO.area(z, m, p=2, q=1, cov=Fraction(1, 2))
    assert r["known"].tolist() == [[True, False], [True, True]]
    assert XO.area(z, m, p=2, q=1, cov=Fraction(1, 4))["known"].all()
    assert XO.area(z, m, p=2, q=1, cov=Fraction(501, 1000))["known"].tolist() == [[False, False], [True, True]]


def test_oracle_return_trip_passes_known_pixels_through():
    rng = np.random.default_rng(1)
    H, W = 41, 53
    z = (900 + 50 * rng.random((H, W))).astype(np.float32)
    m = np.ones((H, W), np.float32)
    m[11:20, 11:30] = 0
    k = XO.known(z, m)
    for p, q in [(2, 1), (10, 3), (1, 2), (3, 10)]:
        fwd = XO.area(z, m, p=p, q=q, cov=Fraction(1, 4)) if p >= q else XO.interp(z, m, p=p, q=q)
        work = fwd["value"].astype(np.float32)
        r = XO.back(work, z, m, None, p, q)
        assert r["value"].shape == (H, W) and np.array_equal(r["passed"], k)
        assert np.array_equal(r["value"][k], z[k].astype(np.float64))
        assert np.isnan(r["value"][15, 20]) and not r["known"][15, 20]       # deep inside the hole nothing exists
        # its rim is reached wherever a working pixel straddles the outline; at 1/2 each native pixel is exactly four working
        # pixels, all of them holes
        assert r["known"][~k].any() == ((p, q) != (1, 2))


# ---- argument validation (nothing here reaches a device) ------------------------------------------------------------
def test_model_cellsize_needs_cellsize_and_valid_scales():
    from mvp_gan.src.evaluate_raster import evaluate_raster
    from mvp_gan.src.inpaint_raster import check_resample_options, inpaint_raster
    from mvp_gan.src.resample import resample_raster
    from mvp_gan.src.utils.raster_dataset import RasterWindowLoader
    z = np.full((64, 64), 900.0, np.float32)
    assert check_resample_options(None, None, 0.5) is None
    assert check_resample_options(1.0, None, 0.5) is None
    assert check_resample_options(1.0, 1.0, 0.5) is None
    assert check_resample_options(0.5, 1.0, 0.5) == 2 and check_resample_options(2, 1, 1) == Fraction(1, 2)
    with pytest.raises(ValueError, match="model_cellsize needs cellsize"):
        inpaint_raster(None, z, model_cellsize=1.0)
    with pytest.raises(ValueError, match="outside"):
        inpaint_raster(None, z, cellsize=20.0, model_cellsize=1.0)
    with pytest.raises(ValueError, match="no fraction"):
        inpaint_raster(None, z, cellsize=1.0, model_cellsize=2 ** 0.5)
    with pytest.raises(ValueError, match="min_coverage"):
        inpaint_raster(None, z, cellsize=1.0, model_cellsize=2.0, min_coverage=0.0)
    with pytest.raises(ValueError, match="min_coverage"):
        inpaint_raster(None, z, min_coverage=1.5)
    with pytest.raises(ValueError, match="outside"):
        evaluate_raster(None, z, cellsize=1.0, model_cellsize=0.1)
    with pytest.raises(ValueError, match="model_cellsize needs cellsize"):
        RasterWindowLoader(z, window=40, model_cellsize=1.0)
    with pytest.raises(ValueError, match="outside"):
        RasterWindowLoader(z, window=40, cellsize=1.0, model_cellsize=20.0)
    with pytest.raises(ValueError, match="outside"):
        resample_raster(z, cellsize=1.0, target_cellsize=0.2)
    with pytest.raises(ValueError, match="min_coverage"):
        resample_raster(z, cellsize=1.0, target_cellsize=2.0, min_coverage=2)
    with pytest.raises(TypeError):
        resample_raster(z, cellsize=1.0)                              # both cell sizes are required
    with pytest.raises(ValueError, match="min_coverage"):
        evaluate_raster(None, z, cellsize=1.0, model_cellsize=2.0, min_coverage=0)
    with pytest.raises(ValueError, match="min_coverage"):
        RasterWindowLoader(z, window=40, cellsize=1.0, model_cellsize=2.0, min_coverage=1.5)
    # the same cell size is no resampling: the loader's host side works as before, without a device
    a = RasterWindowLoader(z, window=40, cellsize=1.0, model_cellsize=1.0, seed=3)
    b = RasterWindowLoader(z, window=40, seed=3)
    assert a.info == b.info and (a.H, a.W) == (64, 64)


def test_held_out_cells_share_no_ground_with_training_blocks():
    """RasterWindowLoader(model_cellsize=...) picks its train / val blocks on the working grid; evaluate_raster cuts its test
    cells on the native grid.  With block and tile converted by native_cells the two agree on the ground: no eligible test
    cell shares a native pixel with the footprint of a working pixel of a train or val block.  Passing the working-pixel
    numbers on unconverted, the mistake this guards against, does not have that property."""
    from mvp_gan.src.evaluate_raster import check_plan, eligible_cells, native_cells
    from mvp_gan.src.utils.raster_dataset import SPLITS, HoleSpec

    def trained_ground(H, W, p, q, B):
        """bool [H][W]: native pixels under a working pixel of a train or val block (working block side B)."""
        Hw, Ww = -(-H * q // p), -(-W * q // p)
        g = np.zeros((H, W), bool)
        for by in range(-(-Hw // B)):
            for bx in range(-(-Ww // B)):
                if (bx - by) % 3 in (SPLITS["train"], SPLITS["val"]):
                    # working pixels I0 .. I1 - 1 cover [I0 p, I1 p) / q, clipped to the raster
                    y0, y1 = by * B * p // q, min(-(-min((by + 1) * B, Hw) * p // q), H)
                    x0, x1 = bx * B * p // q, min(-(-min((bx + 1) * B, Ww) * p // q), W)
                    g[y0:y1, x0:x1] = True
        return g

    def test_ground(H, W, block, tile):
        el = eligible_cells(H, W, "test", block, tile)
        return np.kron(el, np.ones((tile, tile), bool))[:H, :W]

    for (p, q), window, block, (H, W) in [((2, 1), 48, 96, (300, 470)), ((2, 1), 48, 48, (300, 470)),
                                          ((1, 2), 80, 160, (190, 250)), ((10, 3), 48, 96, (700, 1000)),
                                          ((2, 3), 60, 120, (200, 330)), ((4, 1), 40, 80, (500, 1000))]:
        scale = Fraction(p, q)
        bn, tn = native_cells(block, window, scale)
        assert (bn, tn) == (block * p // q, window * p // q) and bn * q == block * p and tn * q == window * p
        check_plan(H, W, "test", bn, tn, HoleSpec())
        tg, te = trained_ground(H, W, p, q, block), test_ground(H, W, bn, tn)
        assert tg.any() and te.any() and not (tg & te).any(), (p, q)
        # together with the working test blocks' ground the raster is covered: nothing is left out of both
        assert (tg | test_ground(H, W, bn, bn)).all()
    # the working-pixel numbers taken for native ones: at scale 2 a working train block spans native blocks of every residue
    assert (trained_ground(300, 470, 2, 1, 96) & test_ground(300, 470, 96, 48)).any()
    assert native_cells(256, 64, None) == (256, 64)
    for block, tile, scale in [(64, 64, Fraction(10, 3)), (96, 50, Fraction(10, 3)), (80, 80, Fraction(2, 3)), (65, 65, Fraction(1, 2))]:
        with pytest.raises(ValueError, match="whole numbers"):
            native_cells(block, tile, scale)
    with pytest.raises(ValueError, match="tile 2048 out of range"):
        check_plan(4096, 4096, "test", *native_cells(512, 128, Fraction(16)), HoleSpec())


def test_cli_flags(capsys):
    from mvp_gan.src import evaluate_raster, inpaint_raster, resample, train_raster
    a = train_raster.build_parser().parse_args(["--dem", "d.asc", "--out", "o.pth"])
    assert a.model_cellsize is None and a.min_coverage == 0.5 and not a.evaluate
    a = train_raster.build_parser().parse_args(["--dem", "d.asc", "--out", "o.pth", "--model-cellsize", "1.5", "--min-coverage",
                                                "0.75", "--evaluate"])
    assert a.model_cellsize == 1.5 and a.min_coverage == 0.75 and a.evaluate
    with pytest.raises(SystemExit):
        train_raster.build_parser().parse_args(["--dem", "d.asc", "--out", "o.pth", "--model-cellsize", "coarse"])
    capsys.readouterr()
    for flag, val in (("--model-cellsize", "2"), ("--fallback", "laplace"), ("--seam", "harmonic")):
        with pytest.raises(SystemExit) as ei:                         # refused by the parser, before any file is opened
            evaluate_raster.main(["--dem", "no.asc", "--pred", "no_p.asc", "--holes", "no_h.png", flag, val])
        assert ei.value.code == 2 and f"{flag} needs --checkpoint" in capsys.readouterr().err
    a = evaluate_raster.build_parser().parse_args(["--dem", "d.asc", "--checkpoint", "c.pth", "--model-cellsize", "2",
                                                   "--min-coverage", "0.3"])
    assert a.model_cellsize == 2.0 and a.min_coverage == 0.3
    assert evaluate_raster.build_parser().parse_args(["--dem", "d.asc", "--checkpoint", "c.pth"]).min_coverage == 0.5
    a = inpaint_raster.build_parser().parse_args(["--dem", "d.asc", "--checkpoint", "c.pth", "--out", "o.asc"])
    assert a.model_cellsize is None and a.min_coverage == 0.5
    a = inpaint_raster.build_parser().parse_args(["--dem", "d.asc", "--checkpoint", "c.pth", "--out", "o.asc",
                                                  "--model-cellsize", "1.0", "--min-coverage", "0.25"])
    assert a.model_cellsize == 1.0 and a.min_coverage == 0.25
    a = evaluate_raster.build_parser().parse_args(["--dem", "d.asc", "--checkpoint", "c.pth", "--model-cellsize", "2"])
    assert a.model_cellsize == 2.0
    a = resample.build_parser().parse_args(["--dem", "d.asc", "--cellsize-out", "1.0", "--out", "o.asc"])
    assert a.cellsize_out == 1.0 and a.min_coverage == 0.5 and a.mask is None
    a = resample.build_parser().parse_args(["--dem", "d.asc", "--cellsize-out", "0.5", "--out", "o.asc", "--mask", "m.png",
                                            "--min-coverage", "1"])
    assert a.cellsize_out == 0.5 and a.min_coverage == 1.0 and a.mask == "m.png"
    for argv in (["--dem", "d.asc", "--out", "o.asc"], ["--dem", "d.asc", "--cellsize-out", "x", "--out", "o.asc"]):
        with pytest.raises(SystemExit):
            resample.build_parser().parse_args(argv)


def test_c_abi_validates_before_any_launch():
    """Null pointers, the direction of each kernel, sizes against the plan and the coverage fraction are refused on the host."""
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    one = 16                                                          # a non-null pointer that is never dereferenced
    area = lambda H, W, p, q, Ho, Wo, cn=1, cd=2, dem=one, out=one, cnt=one, km=None: lib.tg_resample_area(
        dem, None, 0, 0.0, H, W, p, q, cn, cd, None, km, 0, 0.0, Ho, Wo, out, None, cnt, None)
    interp = lambda H, W, p, q, Ho, Wo, dem=one, out=one, cnt=one: lib.tg_resample_interp(
        dem, None, 0, 0.0, H, W, p, q, None, None, 0, 0.0, Ho, Wo, out, None, cnt, None)
    err = lambda: lib.tg_last_error().decode()
    for kw in ({"dem": None}, {"cnt": None}):                         # out may be null: the call then only counts
        assert area(100, 100, 2, 1, 50, 50, **kw) == -1 and "null pointer" in err()
        assert interp(100, 100, 1, 2, 200, 200, **kw) == -1 and "null pointer" in err()
    assert area(100, 100, 1, 2, 200, 200) == -1 and "tg_resample_interp goes to a finer grid" in err()
    assert interp(100, 100, 2, 1, 50, 50) == -1 and "tg_resample_area goes to a coarser grid" in err()
    assert area(100, 100, 17, 1, 6, 6) == -1 and "[1, 16]" in err()
    assert interp(100, 100, 1, 17, 1700, 1700) == -1 and "[1/16, 1]" in err()
    assert area(100, 100, 2, 1, 51, 50) == -1 and "inconsistent with the plan" in err()
    assert area(101, 100, 2, 1, 51, 51) == -1 and "inconsistent with the plan" in err()
    assert interp(100, 100, 1, 2, 200, 201) == -1 and "inconsistent with the plan" in err()
    assert area(100, 100, 2, 1, 0, 50) == -1 and "inconsistent with the plan" in err()
    assert area(0, 100, 2, 1, 1, 50) == -1 and "empty raster" in err()
    assert area(100, 100, 0, 1, 50, 50) == -1 and area(100, 100, 2, 0, 50, 50) == -1 and area(100, 100, 2050, 1025, 50, 50) == -1
    assert area(100, 100, 2, 1, 50, 50, cn=3, cd=2) == -1 and "coverage" in err()
    assert area(100, 100, 2, 1, 50, 50, cn=1, cd=1001) == -1 and "coverage" in err()
    assert area(100, 100, 2, 1, 50, 50, cn=-1) == -1 and "coverage" in err()
    assert area(100, 100, 2, 1, 50, 50, km=one) == -1 and "keep_mask without keep_dem" in err()
    assert area(1 << 30, 100, 2, 1, 1 << 29, 50) == -1 and "too large" in err()


# ---- .asc header ----------------------------------------------------------------------------------------------------
def test_resampled_header():
    from mvp_gan.src.asc import asc_value
    from mvp_gan.src.resample import resample_plan, resampled_header
    hdr = [("ncols", "317"), ("nrows", "203"), ("xllcorner", "500000.5"), ("yllcorner", "4100000"), ("cellsize", "0.3"),
           ("NODATA_value", "-9999")]
    pl = resample_plan(203, 317, 10, 3)
    out = resampled_header(hdr, (203, 317), 0.3, 1.0, (pl.Ho, pl.Wo))
    assert [k for k, _ in out] == [k for k, _ in hdr]
    assert (asc_value(out, "ncols"), asc_value(out, "nrows")) == ("96", "61") and float(asc_value(out, "cellsize")) == 1.0
    assert asc_value(out, "xllcorner") == "500000.5" and asc_value(out, "NODATA_value") == "-9999"
    # the top edge stays where it was: yll' + Ho c' == yll + H c
    assert float(asc_value(out, "yllcorner")) + 61 * 1.0 == pytest.approx(4100000 + 203 * 0.3, abs=1e-6)
    assert float(asc_value(out, "yllcorner")) <= 4100000                # the clipped last row reaches below the old edge
    # the centre form keeps its form and describes the same grid
    hc = [("ncols", "100"), ("nrows", "80"), ("xllcenter", "10.5"), ("yllcenter", "20.5"), ("cellsize", "1")]
    oc = resampled_header(hc, (80, 100), 1.0, 0.5, (160, 200))
    assert float(asc_value(oc, "xllcenter")) == 10.25 and float(asc_value(oc, "yllcenter")) == 20.25
    assert (asc_value(oc, "ncols"), asc_value(oc, "nrows"), float(asc_value(oc, "cellsize"))) == ("200", "160", 0.5)
