"""CPU checks of the seam correction (mvp_gan/src/seam_correct.py, csrc/seam.hip): properties of the numpy oracle in
tests/seam_oracle.py (exact on planes at order 1 and not at order 0, better than the uncorrected fill on a synthetic fill with
an offset per hole, strokes, the order-0 fallback, raster borders, unfilled patches), host-side rejection by the C entry points
and the Python API, the new CLI flags and the ctypes table, all without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import raster_oracle as RO
from tests import seam_oracle as SO
from tests import vfill_oracle as VO


def _plane(H, W, a=900.0, b=0.31, c=-0.17):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return a + b * x + c * y


def _harmonic_error(H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = (x - W / 2) / 20.0, (y - H / 2) / 20.0
    return 1.3 + 0.8 * x - 0.5 * y + 0.4 * (x * x - y * y)


def _cg_solve(z, known):
    """The fill of vfill_oracle.solve by conjugate gradients (numpy, matrix-free): for components too large for a dense solve."""
    z = np.asarray(z, np.float64)
    unk = ~known

    def nsum(v):
        s = np.zeros_like(v)
        s[1:, :] += v[:-1, :]
        s[:-1, :] += v[1:, :]
        s[:, 1:] += v[:, :-1]
        s[:, :-1] += v[:, 1:]
        return s

    deg = nsum(np.ones_like(z))
    A = lambda v: np.where(unk, deg * v - nsum(v), 0.0)
    u0 = np.where(known, z, 0.0)
    b = np.where(unk, nsum(u0), 0.0)
    x = np.zeros_like(z)
    r = b - A(x)
    p = r.copy()
    rr = float((r * r).sum())
    stop = 1e-24 * max(float((b * b).sum()), 1e-300)
    for _ in range(20000):
        if rr <= stop:
            break
        Ap = A(p)
        al = rr / float((p * Ap).sum())
        x += al * p
        r -= al * Ap
        rn = float((r * r).sum())
        p = r + (rn / rr) * p
        rr = rn
    assert rr <= stop, "conjugate gradients did not converge"
    return u0 + x


# ---- the oracle -----------------------------------------------------------------------------------------------------
def _planar_case():
    H, W = 90, 120
    truth = _plane(H, W)
    hole = VO.disc(H, W, 30, 35, 14) | VO.disc(H, W, 60, 85, 20) | VO.disc(H, W, 20, 95, 6)
    filled = np.where(hole, truth + _harmonic_error(H, W), np.nan)
    return truth, hole, filled


def test_order_1_is_exact_on_planes():
    truth, hole, filled = _planar_case()
    out, info = SO.correct(truth, filled, (~hole).astype(np.float32), order=1)
    rng = truth.max() - truth.min()
    assert info["ring"] > 0 and info["interior"] > 0 and info["unfilled"] == 0
    assert np.abs(out - truth).max() <= 1e-9 * rng
    assert info["max_delta"] > 0.5                      # the fill was off by metres


def test_order_0_is_not_exact_on_planes():
    truth, hole, filled = _planar_case()
    out, _ = SO.correct(truth, filled, (~hole).astype(np.float32), order=0)
    rng = truth.max() - truth.min()
    assert np.abs(out - truth)[hole].max() > 1e-3 * rng
    # yet far better than the fill itself
    assert np.abs(out - truth)[hole].max() < 0.5 * np.abs(filled - truth)[hole].max()


@pytest.mark.parametrize("order", [1, 0])
def test_correction_beats_the_uncorrected_fill(order):
    H, W = 600, 800
    truth = RO.terrain(H, W, 3)
    hole = RO.disc_holes(H, W, 0.2, 5)
    rng = np.random.default_rng(17)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    err = 0.8 * np.sin(x / 37.0 + 0.4) * np.cos(y / 29.0 - 1.1)          # a smooth error field
    for comp in VO.components(hole):                                     # an offset per hole
        err.ravel()[comp] += rng.normal(0, 1.5)
    filled = np.where(hole, truth.astype(np.float64) + err, np.nan).astype(np.float32)
    D, k, ring, interior, unfilled = SO.delta(truth, filled, (~hole).astype(np.float32), order=order)
    assert not unfilled.any() and np.array_equal(k, ~hole) and np.array_equal(ring | interior, hole)
    Ds = _cg_solve(D, ~interior)
    out = np.where(hole, filled.astype(np.float64) + Ds, truth)
    r8 = SO.ring8(k, hole)
    rmse = lambda a, sel: math.sqrt(float(((a - truth)[sel] ** 2).mean()))
    raw_h, raw_r, cor_h, cor_r = rmse(filled, hole), rmse(filled, r8), rmse(out, hole), rmse(out, r8)
    print(f"order {order}: hole RMSE {raw_h:.3f} -> {cor_h:.3f} m, ring RMSE {raw_r:.3f} -> {cor_r:.3f} m")
    assert cor_h < raw_h and cor_r < raw_r


def test_one_pixel_strokes_are_all_ring():
    H, W = 30, 40
    z = RO.terrain(H, W, 1)
    hole = np.zeros((H, W), bool)
    hole[10, 5:30] = True
    hole[15:28, 33] = True
    filled = np.where(hole, z + 2.5, np.nan).astype(np.float32)
    m = (~hole).astype(np.float32)
    z64 = z.astype(np.float64)
    for order in (0, 1):
        out, info = SO.correct(z, filled, m, order=order)
        assert info["interior"] == 0 and info["ring"] == int(hole.sum())
        D = info["D"]
        assert np.array_equal(out[hole], filled.astype(np.float64)[hole] + D[hole])
        # a pixel in the middle of the horizontal stroke sees the rows above and below
        up = 2 * z64[9, 17] - z64[8, 17] if order else z64[9, 17]
        dn = 2 * z64[11, 17] - z64[12, 17] if order else z64[11, 17]
        assert abs(out[10, 17] - 0.5 * (up + dn)) <= 1e-9
        # the stroke's left end also sees its left neighbour
        lf = 2 * z64[10, 4] - z64[10, 3] if order else z64[10, 4]
        up = 2 * z64[9, 5] - z64[8, 5] if order else z64[9, 5]
        dn = 2 * z64[11, 5] - z64[12, 5] if order else z64[11, 5]
        assert abs(out[10, 5] - (up + lf + dn) / 3) <= 1e-9


def test_order_1_falls_back_without_a_known_second_neighbour():
    z = RO.terrain(7, 7, 2)
    hole = np.ones((7, 7), bool)
    hole[3, 3] = False                                   # one known pixel: no direction has a known second pixel
    filled = np.where(hole, z - 4.0, np.nan).astype(np.float32)
    o1, i1 = SO.correct(z, filled, (~hole).astype(np.float32), order=1)
    o0, i0 = SO.correct(z, filled, (~hole).astype(np.float32), order=0)
    assert i1["ring"] == 4 and i1["interior"] == 44
    assert np.array_equal(o1, o0)
    for y, x in ((2, 3), (3, 2), (3, 4), (4, 3)):
        assert o1[y, x] == float(z[3, 3])
    # a second known pixel behind the first switches that one direction to order 1
    hole[3, 4] = False
    filled = np.where(hole, z - 4.0, np.nan).astype(np.float32)
    o1, _ = SO.correct(z, filled, (~hole).astype(np.float32), order=1)
    assert abs(o1[3, 2] - (2.0 * float(z[3, 3]) - float(z[3, 4]))) <= 1e-12
    assert o1[2, 3] == float(z[3, 3])


def test_holes_on_the_border_and_in_a_corner():
    H, W = 24, 31
    z = RO.terrain(H, W, 3)
    hole = np.zeros((H, W), bool)
    hole[:5, :7] = True                                  # the top-left corner
    hole[10:16, W - 4:] = True                           # the right edge
    hole[H - 1, 12:20] = True                            # a stroke on the bottom edge
    filled = np.where(hole, z + 1.0, np.nan).astype(np.float32)
    out, info = SO.correct(z, filled, (~hole).astype(np.float32), order=1)
    k, ring, interior, unfilled = SO.classify(z, filled, (~hole).astype(np.float32))
    assert info["ring"] == int(ring.sum()) and info["interior"] == int(interior.sum()) and not unfilled.any()
    assert interior[0, 0] and ring[4, 0] and ring[0, 6] and interior[3, 5]
    assert np.isfinite(out).all()
    z64 = z.astype(np.float64)
    assert abs(out[4, 0] - (2 * z64[5, 0] - z64[6, 0])) <= 1e-9            # only `down` is known; left is outside
    assert abs(out[H - 1, 15] - (2 * z64[H - 2, 15] - z64[H - 3, 15])) <= 1e-9
    # the interior of the delta is harmonic with a natural border
    D = out - np.where(hole, filled.astype(np.float64), z64)
    assert np.abs(VO.residual(D, ~interior)).max() <= 1e-9
    # a constant offset is removed exactly wherever the ring is exact: on a plane the corner comes back too
    p = _plane(H, W)
    out, _ = SO.correct(p, np.where(hole, p + 1.0, np.nan), (~hole).astype(np.float32), order=1)
    assert np.abs(out - p).max() <= 1e-9 * (p.max() - p.min())


def test_an_unfilled_region_next_to_a_filled_one():
    H, W = 30, 40
    z = RO.terrain(H, W, 4)
    hole = np.zeros((H, W), bool)
    hole[5:25, 5:35] = True
    filled = np.where(hole, z + 3.0, np.nan).astype(np.float32)
    filled[5:25, 18:35] = np.nan                         # the right part was never filled
    filled[12, 10] = np.inf                              # nor was this pixel
    m = (~hole).astype(np.float32)
    out, info = SO.correct(z, filled, m, order=1)
    k, ring, interior, unfilled = SO.classify(z, filled, m)
    assert info["unfilled"] == int(unfilled.sum()) == 20 * 17 + 1
    assert np.isnan(out[unfilled]).all() and np.isfinite(out[~unfilled]).all()
    assert interior[10, 17] and not ring[10, 17]         # next to unfilled pixels only: not a ring pixel
    assert info["D"][12, 10] == 0 and info["D"][10, 20] == 0
    # the unfilled pixels are fixed at delta 0: the correction fades towards them
    D = out - filled.astype(np.float64)
    assert abs(D[10, 17]) < abs(D[10, 5])
    assert np.array_equal(out[k], z.astype(np.float64)[k])


def test_nothing_known_and_no_holes():
    z = RO.terrain(9, 11, 5)
    g = (z + 1).astype(np.float32)
    out, info = SO.correct(z, g, np.zeros(z.shape, np.float32))
    assert info["ring"] == 0 and info["interior"] == z.size and np.array_equal(out, g.astype(np.float64))
    out, info = SO.correct(z, g)
    assert (info["ring"], info["interior"], info["unfilled"], info["max_delta"]) == (0, 0, 0, 0.0)
    assert np.array_equal(out, z.astype(np.float64))


# ---- host-side rejection --------------------------------------------------------------------------------------------
def _lib():
    from tg_hip import lib as L
    return L, L.load()


def test_lib_table_holds_both_entry_points():
    L, lib = _lib()
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert L.SIGNATURES["tg_seam_delta"] == (I, [P, P, I, F, P, I, I, I, P, P, P])
    assert L.SIGNATURES["tg_seam_apply"] == (I, [P, P, I, F, P, P, I, I, P, P])
    assert lib.tg_seam_delta.argtypes == L.SIGNATURES["tg_seam_delta"][1]
    assert lib.tg_seam_apply.argtypes == L.SIGNATURES["tg_seam_apply"][1]


def test_c_entry_points_reject_without_gpu():
    _, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(5)]       # never dereferenced: every call below fails validation first

    def err(rc, msg):
        assert rc == -1 and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15)):
        err(lib.tg_seam_delta(f[0], None, 0, 0.0, f[1], H, W, 1, f[2], f[3], None), b"H*W < 2^31")
        err(lib.tg_seam_apply(f[0], None, 0, 0.0, f[1], f[2], H, W, f[3], None), b"H*W < 2^31")
    for order in (-1, 2, 7):
        err(lib.tg_seam_delta(f[0], None, 0, 0.0, f[1], 8, 8, order, f[2], f[3], None), b"order")
    for a in range(4):
        p = [f[0], f[1], f[2], f[3]]
        p[a] = None
        err(lib.tg_seam_delta(p[0], None, 0, 0.0, p[1], 8, 8, 1, p[2], p[3], None), b"tg_seam_delta: null pointer")
        err(lib.tg_seam_apply(p[0], None, 0, 0.0, p[1], p[2], 8, 8, p[3], None), b"tg_seam_apply: null pointer")


@pytest.mark.parametrize("kw,match", [
    (dict(order=2), "order"),
    (dict(order=-1), "order"),
    (dict(order=None), "order"),
    (dict(order=True), "order"),
    (dict(order=0.5), "order"),
    (dict(tol=-1e-3), "tol"),
    (dict(tol=math.nan), "tol"),
    (dict(tol=math.inf), "tol"),
    (dict(tol="x"), "tol"),
    (dict(max_cycles=0), "max_cycles"),
    (dict(max_cycles=2.5), "max_cycles"),
    (dict(max_cycles=True), "max_cycles"),
])
def test_python_rejects_bad_options(kw, match):
    from mvp_gan.src.seam_correct import correct_seams
    z = np.zeros((8, 8), np.float32)
    with pytest.raises(ValueError, match=match):
        correct_seams(z, z, **kw)


def test_python_rejects_bad_shapes():
    from mvp_gan.src.seam_correct import correct_seams
    z = np.zeros((4, 4), np.float32)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        correct_seams(np.zeros((2, 3, 4), np.float32), z)
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        correct_seams(np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="filled"):
        correct_seams(z, np.zeros((4, 5), np.float32))
    with pytest.raises(ValueError, match="mask"):
        correct_seams(z, z, np.ones((5, 4), np.float32))

    class Big:
        shape = (1 << 16, 1 << 15)
    with pytest.raises(ValueError, match="2\\^31"):
        correct_seams(Big(), Big())


def test_inpaint_and_evaluate_reject_unknown_seam_options():
    from mvp_gan.src.inpaint_raster import check_seam_options
    check_seam_options(None, 1)
    check_seam_options("harmonic", 0)
    with pytest.raises(ValueError, match="seam"):
        check_seam_options("poisson", 1)
    for o in (2, -1, None, True, 0.5):
        with pytest.raises(ValueError, match="seam_order"):
            check_seam_options("harmonic", o)
    with pytest.raises(ValueError, match="evaluate_raster: seam"):
        check_seam_options("x", 1, who="evaluate_raster")


# ---- CLI flags ------------------------------------------------------------------------------------------------------
def test_seam_correct_cli_flags_parse():
    from mvp_gan.src.seam_correct import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--filled", "f.asc", "--out", "o.asc", "--mask", "m.png", "--nodata", "-9999",
                                   "--order", "0", "--tol", "0.01", "--max-cycles", "7"])
    assert (a.dem, a.filled, a.out, a.mask, a.nodata, a.order, a.tol, a.max_cycles) == \
        ("in.asc", "f.asc", "o.asc", "m.png", -9999.0, 0, 0.01, 7)
    d = build_parser().parse_args(["--dem", "in.asc", "--filled", "f.asc", "--out", "o.asc"])
    assert (d.mask, d.nodata, d.order, d.tol, d.max_cycles) == (None, None, 1, None, 200)
    for bad in (["--dem", "in.asc", "--out", "o.asc"], ["--dem", "in.asc", "--filled", "f.asc"],
                ["--dem", "in.asc", "--filled", "f.asc", "--out", "o.asc", "--order", "2"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_inpaint_raster_cli_seam_flags_parse():
    from mvp_gan.src.inpaint_raster import build_parser
    base = ["--dem", "in.asc", "--checkpoint", "ck.pth", "--out", "o.asc"]
    d = build_parser().parse_args(base)
    assert (d.seam, d.seam_order, d.fallback) == (None, 1, None)
    a = build_parser().parse_args(base + ["--seam", "harmonic", "--seam-order", "0", "--fallback", "laplace"])
    assert (a.seam, a.seam_order, a.fallback) == ("harmonic", 0, "laplace")
    for bad in (["--seam", "poisson"], ["--seam", "harmonic", "--seam-order", "2"], ["--seam"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(base + bad)


def test_evaluate_raster_cli_seam_flag_parses_and_needs_a_checkpoint():
    from mvp_gan.src.evaluate_raster import build_parser, main
    base = ["--dem", "/nonexistent/in.asc"]
    assert build_parser().parse_args(base + ["--checkpoint", "ck.pth"]).seam is None
    assert build_parser().parse_args(base + ["--checkpoint", "ck.pth", "--seam", "harmonic"]).seam == "harmonic"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--checkpoint", "ck.pth", "--seam", "poisson"])
    with pytest.raises(SystemExit):
        main(base + ["--pred", "p.asc", "--holes", "h.png", "--seam", "harmonic"])
    with pytest.raises(FileNotFoundError):                     # the flag parses; the raster is read next
        main(base + ["--checkpoint", "ck.pth", "--seam", "harmonic"])
