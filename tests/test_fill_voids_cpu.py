"""CPU checks of the harmonic void fill (mvp_gan/src/fill_voids.py, csrc/voidfill.hip): the numpy oracle against scipy and the
closed-form harmonic fields, the border rule, the level plan and the workspace query against its host mirror, host-side
rejection by the C entry points and the Python API, and the new CLI flags, all without a GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import vfill_oracle as VO


def _terrain(H, W, seed):
    rng = np.random.default_rng(seed)
    return (VO.harmonic_field(H, W, (80, 3, -2, 1.5, 0.7, 0.05), W / 2, H / 2, max(H, W) / 2)
            + rng.normal(0, 0.4, (H, W))).astype(np.float32)


def _random_holes(H, W, seed, n):
    rng = np.random.default_rng(seed)
    u = np.zeros((H, W), bool)
    for _ in range(n):
        u |= VO.disc(H, W, rng.integers(0, H), rng.integers(0, W), rng.integers(2, 9))
    return ~u


# ---- the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,seed", [(60, 90, 0), (121, 77, 1)])
def test_oracle_matches_scipy_spsolve(H, W, seed):
    sp = pytest.importorskip("scipy.sparse")
    spla = pytest.importorskip("scipy.sparse.linalg")
    z = _terrain(H, W, seed)
    k = _random_holes(H, W, seed, 25)
    k[0, :W // 3] = False                                  # a hole on the raster border
    u = VO.solve(z, k)
    idx = -np.ones(H * W, np.int64)
    unk = np.flatnonzero(~k.ravel())
    idx[unk] = np.arange(unk.size)
    rows, cols, vals = [], [], []
    b = np.zeros(unk.size)
    zf = z.astype(np.float64).ravel()
    for j, i in enumerate(unk):
        y, x = divmod(int(i), W)
        for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= yy < H and 0 <= xx < W:
                q = yy * W + xx
                rows.append(j); cols.append(j); vals.append(1.0)
                if idx[q] >= 0:
                    rows.append(j); cols.append(idx[q]); vals.append(-1.0)
                else:
                    b[j] += zf[q]
    A = sp.csr_matrix((vals, (rows, cols)), shape=(unk.size, unk.size))
    ref = spla.spsolve(A, b)
    np.testing.assert_allclose(u.ravel()[unk], ref, rtol=0, atol=1e-9)
    assert np.array_equal(u[k], z[k].astype(np.float64))


@pytest.mark.parametrize("coef", [(5, 1, -2, 0.3, 0.2, 0.01), (-40, 0, 0, 2, -1, 0.1)])
def test_oracle_reproduces_closed_form_fields(coef):
    H, W = 70, 90
    f = VO.harmonic_field(H, W, coef, 45, 35, 20)
    k = ~(VO.disc(H, W, 30, 40, 14) | VO.disc(H, W, 55, 70, 8))       # holes off the raster border
    u = VO.solve(f, k)
    np.testing.assert_allclose(u, f, rtol=0, atol=1e-9 * np.abs(f).max())


def test_closed_form_fields_satisfy_the_5_point_equation():
    f = VO.harmonic_field(40, 50, (1, 2, 3, 4, 5, 6), 20, 25, 7)
    lap = f[:-2, 1:-1] + f[2:, 1:-1] + f[1:-1, :-2] + f[1:-1, 2:] - 4 * f[1:-1, 1:-1]
    assert np.abs(lap).max() <= 1e-9 * np.abs(f).max()


def test_oracle_border_rule_is_natural():
    # a hole along the top edge and into a corner: the border pixels average their in-raster neighbours only
    H, W = 30, 40
    z = _terrain(H, W, 3)
    k = np.ones((H, W), bool)
    k[:6, :15] = False
    k[20:, 33:] = False
    u = VO.solve(z, k)
    assert np.abs(VO.residual(u, k)).max() <= 1e-9
    # the corner pixel has two neighbours: u = mean of them
    assert abs(u[H - 1, W - 1] - 0.5 * (u[H - 2, W - 1] + u[H - 1, W - 2])) <= 1e-9


def test_oracle_empty_known_is_nan_and_one_known_is_constant():
    z = _terrain(12, 9, 4)
    assert np.isnan(VO.solve(z, np.zeros(z.shape, bool))).all()
    k = np.zeros(z.shape, bool)
    k[3, 4] = True
    np.testing.assert_allclose(VO.solve(z, k), float(z[3, 4]), atol=1e-9)


def test_oracle_known_mask_rule():
    z = np.array([[1, np.nan, np.inf], [-np.inf, -9999, 5]], np.float32)
    m = np.array([[1, 1, 1], [1, 1, 0]], np.float32)
    assert VO.known_mask(z, m, -9999).tolist() == [[True, False, False], [False, False, False]]
    assert VO.known_mask(z, None, float("nan")).tolist() == [[True, False, False], [False, True, True]]


# ---- level plan and workspace ---------------------------------------------------------------------------------------
def test_level_plan():
    from mvp_gan.src.fill_voids import vfill_levels
    assert vfill_levels(1, 1) == [(1, 1)]
    assert vfill_levels(16, 16) == [(16, 16)]
    assert vfill_levels(17, 3) == [(17, 3), (9, 2)]
    assert vfill_levels(8192, 8192)[-1] == (16, 16) and len(vfill_levels(8192, 8192)) == 10
    assert vfill_levels(8193, 8191)[1] == (4097, 4096)
    for H, W in ((1, 100000), (257, 129), (1500, 2100)):
        lv = vfill_levels(H, W)
        assert max(lv[-1]) <= 16 and all(max(a) > 16 for a in lv[:-1])
        assert all((h2, w2) == ((h + 1) // 2, (w + 1) // 2) for (h, w), (h2, w2) in zip(lv, lv[1:]))


def _lib():
    from tg_hip import lib as L
    return L, L.load()


SIZES = [(1, 1), (1, 2), (2, 1), (16, 16), (17, 16), (33, 65), (64, 64), (65, 64), (37, 53), (257, 129), (1500, 2100),
         (4096, 4096), (4097, 4095), (8192, 8192), (8193, 8191), (1, 300000), (300000, 1)]


@pytest.mark.parametrize("H,W", SIZES)
def test_ws_query_covers_the_mirror_layout(H, W):
    from mvp_gan.src.fill_voids import vfill_layout, vfill_levels
    _, lib = _lib()
    levels, total = vfill_layout(H, W)
    assert lib.tg_vfill_levels(H, W) == len(vfill_levels(H, W)) == len(levels)
    nb = lib.tg_vfill_ws_bytes(H, W)
    assert nb >= total
    # every region fits and none overlaps: flags, tile list, two value buffers (+ rhs on coarse levels)
    spans = [(0, 256)]
    for l, v in enumerate(levels):
        n = v["H"] * v["W"]
        spans += [(v["flags"], n), (v["list"], 4 * v["tiles"]), (v["u0"], 4 * n), (v["u1"], 4 * n)]
        if l:
            spans.append((v["f"], 4 * n))
    spans.sort()
    for (a, na), (b, _) in zip(spans, spans[1:]):
        assert a + na <= b
    assert spans[-1][0] + spans[-1][1] <= nb
    assert all(o % 256 == 0 for o, _ in spans)


def test_ws_query_rejects_bad_shapes():
    _, lib = _lib()
    for H, W in ((0, 5), (5, 0), (-1, 3), (1 << 16, 1 << 15)):
        assert lib.tg_vfill_ws_bytes(H, W) == 0
        assert lib.tg_vfill_levels(H, W) == 0


# ---- host-side rejection --------------------------------------------------------------------------------------------
def test_c_entry_points_reject_without_gpu():
    L, lib = _lib()
    f = [C.c_void_p(0x1000 * (i + 1)) for i in range(6)]
    ws = C.c_void_p(0x100000)                                # 256-byte aligned, never dereferenced

    def err(rc, msg, code=(-1, -3)):
        assert rc in code and msg in lib.tg_last_error(), (rc, lib.tg_last_error())

    nb = lib.tg_vfill_ws_bytes(8, 8)
    for H, W in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15)):
        err(lib.tg_vfill_setup(f[0], None, 0, 0.0, H, W, ws, 1 << 30, f[1], None), b"H*W < 2^31")
        err(lib.tg_vfill_cycle(H, W, ws, 1 << 30, f[1], None), b"H*W < 2^31")
        err(lib.tg_vfill_finish(f[0], H, W, ws, 1 << 30, f[1], None), b"H*W < 2^31")
    err(lib.tg_vfill_setup(None, None, 0, 0.0, 8, 8, ws, nb, f[1], None), b"null pointer")
    err(lib.tg_vfill_setup(f[0], None, 0, 0.0, 8, 8, ws, nb, None, None), b"null pointer")
    err(lib.tg_vfill_setup(f[0], None, 0, 0.0, 8, 8, None, nb, f[1], None), b"null pointer")
    err(lib.tg_vfill_cycle(8, 8, ws, nb, None, None), b"null pointer")
    err(lib.tg_vfill_cycle(8, 8, None, nb, f[1], None), b"null pointer")
    err(lib.tg_vfill_finish(None, 8, 8, ws, nb, f[1], None), b"null pointer")
    err(lib.tg_vfill_finish(f[0], 8, 8, ws, nb, None, None), b"null pointer")
    for call in (lambda b: lib.tg_vfill_setup(f[0], None, 0, 0.0, 8, 8, ws, b, f[1], None),
                 lambda b: lib.tg_vfill_cycle(8, 8, ws, b, f[1], None),
                 lambda b: lib.tg_vfill_finish(f[0], 8, 8, ws, b, f[1], None)):
        err(call(nb - 1), b"workspace", (-3,))
        err(call(0), b"workspace", (-3,))
    err(lib.tg_vfill_setup(f[0], None, 0, 0.0, 8, 8, C.c_void_p(0x100004), nb, f[1], None), b"aligned")
    # a workspace sized for a smaller raster is short for a larger one
    err(lib.tg_vfill_cycle(300, 200, ws, lib.tg_vfill_ws_bytes(150, 100), f[1], None), b"workspace", (-3,))


@pytest.mark.parametrize("kw,match", [
    (dict(method="idw"), "method"),
    (dict(method=None), "method"),
    (dict(tol=-1e-3), "tol"),
    (dict(tol=math.nan), "tol"),
    (dict(tol=math.inf), "tol"),
    (dict(tol="x"), "tol"),
    (dict(max_cycles=0), "max_cycles"),
    (dict(max_cycles=-3), "max_cycles"),
    (dict(max_cycles=2.5), "max_cycles"),
    (dict(max_cycles=True), "max_cycles"),
])
def test_python_rejects_bad_options(kw, match):
    from mvp_gan.src.fill_voids import fill_voids
    with pytest.raises(ValueError, match=match):
        fill_voids(np.zeros((8, 8), np.float32), **kw)


@pytest.mark.parametrize("cellsize", [None, 0.0, -1.0, math.nan, math.inf, "a"])
def test_python_rejects_objects_without_cellsize(cellsize):
    from mvp_gan.src.fill_voids import fill_voids
    from mvp_gan.src.object_mask import ObjectSpec
    with pytest.raises(ValueError, match="cellsize"):
        fill_voids(np.zeros((8, 8), np.float32), objects=ObjectSpec(), cellsize=cellsize)


def test_python_rejects_bad_shapes():
    from mvp_gan.src.fill_voids import fill_voids
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        fill_voids(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        fill_voids(np.zeros((0, 4), np.float32))
    with pytest.raises(ValueError, match="mask"):
        fill_voids(np.zeros((4, 4), np.float32), np.ones((4, 5), np.float32))

    class Big:
        shape = (1 << 16, 1 << 15)
    with pytest.raises(ValueError, match="2\\^31"):
        fill_voids(Big())


def test_inpaint_and_evaluate_reject_unknown_fill_options():
    from mvp_gan.src.evaluate_raster import _check_fill_options
    with pytest.raises(ValueError, match="baseline"):
        _check_fill_options("idw", None)
    with pytest.raises(ValueError, match="fallback"):
        _check_fill_options(None, "nearest")
    _check_fill_options(None, None)
    _check_fill_options("laplace", "laplace")


# ---- CLI flags ------------------------------------------------------------------------------------------------------
def test_fill_voids_cli_flags_parse():
    from mvp_gan.src.fill_voids import build_parser
    a = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc", "--mask", "m.png", "--nodata", "-9999", "--tol", "0.01",
                                   "--max-cycles", "7", "--remove-objects", "--max-size", "30"])
    assert (a.dem, a.out, a.mask, a.nodata, a.tol, a.max_cycles, a.remove_objects, a.max_size) == \
        ("in.asc", "o.asc", "m.png", -9999.0, 0.01, 7, True, 30.0)
    d = build_parser().parse_args(["--dem", "in.asc", "--out", "o.asc"])
    assert (d.tol, d.max_cycles, d.remove_objects, d.nodata) == (None, 50, False, None)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--dem", "in.asc"])


@pytest.mark.parametrize("module,base", [
    ("inpaint_raster", ["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth", "--out", "o.asc"]),
    ("evaluate_raster", ["--dem", "/nonexistent/in.asc", "--checkpoint", "ck.pth"]),
])
def test_fallback_flag_parses(module, base):
    import importlib
    mod = importlib.import_module(f"mvp_gan.src.{module}")
    with pytest.raises(SystemExit):
        mod.main(base + ["--fallback", "nearest"])
    with pytest.raises(FileNotFoundError):                     # the flag parses; the raster is read next
        mod.main(base + ["--fallback", "laplace"])


@pytest.mark.parametrize("extra", [["--checkpoint", "ck.pth"], ["--pred", "p.asc", "--holes", "h.png"]])
def test_evaluate_baseline_flag_parses_in_both_modes(extra):
    from mvp_gan.src.evaluate_raster import main
    base = ["--dem", "/nonexistent/in.asc"] + extra
    with pytest.raises(SystemExit):
        main(base + ["--baseline", "idw"])
    with pytest.raises(FileNotFoundError):
        main(base + ["--baseline", "laplace"])


def test_evaluate_fallback_needs_checkpoint():
    from mvp_gan.src.evaluate_raster import main
    with pytest.raises(SystemExit):
        main(["--dem", "/nonexistent/in.asc", "--pred", "p.asc", "--holes", "h.png", "--fallback", "laplace"])
