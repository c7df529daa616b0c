"""CPU checks of the texture row: the numpy oracle of tests/texture_oracle.py on analytic cases, the pure
halves of the row (assemble_texture, texture_summary, assemble_compare), the signatures, the refusals that need no GPU and the
parsers.  Every analytic case is integer-valued, so every sum is exact in float64 and compared with ==."""
import inspect
import json
import math

import numpy as np
import pytest

from tests import texture_oracle as TO


def _plane(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (3 * x - 2 * y + 7).astype(np.float32)


def _span(lo, hi, n, h):
    """How many of the centres lo .. hi - 1 along a side of n pixels have both arms at lag h inside."""
    return max(0, min(hi - 1, n - 1 - h) - max(lo, h) + 1)


def _closed_counts(H, W, y0, y1, x0, x1, octaves=5):
    """The triples of a rectangular hole [y0:y1, x0:x1] in a raster without unknown pixels, per scale: a step along x needs the
    arms inside along x only, a step along y along y only, a diagonal step along both."""
    out = []
    for j in range(octaves):
        h = 1 << j
        ny, nx = _span(y0, y1, H, h), _span(x0, x1, W, h)
        out += [(y1 - y0) * nx + ny * (x1 - x0), 2 * ny * nx]
    return out + [0] * (2 * (5 - octaves))


def _report(z, p, sel, known, octaves=5, cellsize=1.0):
    from mvp_gan.src.evaluate_raster import assemble_texture
    counts, sums, _ = TO.spectrum(z, p, sel, known, octaves)
    return assemble_texture(counts.tolist(), sums.tolist(), cellsize=cellsize, octaves=octaves), counts, sums


# ---- the oracle on analytic cases ----------------------------------------------------------------------------------------
def test_plane():
    H, W = 41, 53
    z = _plane(H, W)
    sel = np.zeros((H, W), np.uint8)
    sel[5:36, 4:50] = 1
    known = np.ones((H, W), np.uint8)
    d, counts, sums = _report(z, z + 0, sel, known)
    assert counts.tolist() == _closed_counts(H, W, 5, 36, 4, 50)
    # the same numbers written out.  Diagonal: 2852, 2852, 2790, 1850, 378.  Axial: a step along x and a step along y are
    # separate triples, each with its own arms, so from lag 4 on, where the hole's 46 columns lose more centres than its 31 rows,
    # the axial class keeps more triples than the diagonal one: 31 * nx + ny * 46.
    assert counts[1::2].tolist() == [2852, 2852, 2790, 1850, 378]
    assert counts[0::2].tolist() == [2852, 2852, 31 * 45 + 31 * 46, 31 * 37 + 25 * 46, 31 * 21 + 9 * 46]
    assert (sums == 0).all()
    for s in d["scales"]:
        assert s["truth_rms"] == 0.0 and s["fill_rms"] == 0.0 and s["ratio"] is None and s["corr"] is None
    assert d["scales_scored"] == 0 and d["log_ratio_rms"] is None


def test_quadratic():
    """p = z + 2 x^2: the second difference along x is 4 h^2, along y 0, along both diagonals 4 h^2.  The hole keeps 16 px from
    every border, so both axial steps have the same number of triples."""
    H, W = 80, 90
    z = _plane(H, W)
    x = np.arange(W, dtype=np.float32)[None, :]
    p = z + 2 * x * x
    sel = np.zeros((H, W), np.uint8)
    sel[20:60, 20:70] = 1
    d, counts, sums = _report(z, p, sel, np.ones((H, W), np.uint8), cellsize=2.0)
    n = 40 * 50
    assert counts.tolist() == [2 * n] * 10 == _closed_counts(H, W, 20, 60, 20, 70)
    for j in range(5):
        h = 1 << j
        ax, dg = d["scales"][2 * j], d["scales"][2 * j + 1]
        assert (ax["lag_px"], ax["class"], ax["lag_m"]) == (h, "axial", 2.0 * h)
        assert (dg["lag_px"], dg["class"], dg["lag_m"]) == (h, "diagonal", 2.0 * h * math.sqrt(2.0))
        assert sums[2 * j].tolist() == [0.0, n * 16.0 * h ** 4, 0.0] and sums[2 * j + 1].tolist() == [0.0, 2 * n * 16.0 * h ** 4, 0.0]
        assert ax["fill_rms"] == math.sqrt(8.0 * h ** 4) and ax["fill_rms"] == pytest.approx(4 * h * h / math.sqrt(2.0), rel=1e-15)
        assert dg["fill_rms"] == 4.0 * h * h
        assert ax["truth_rms"] == 0.0 and ax["ratio"] is None and ax["corr"] is None


def test_checkerboard():
    """p = z + a (-1)^(x + y) everywhere: a step of one pixel along an axis flips the sign, every other step keeps it."""
    H, W, a = 40, 37, 3.0
    z = _plane(H, W)
    y, x = np.mgrid[0:H, 0:W]
    p = (z + a * (1 - 2 * ((x + y) & 1))).astype(np.float32)
    d, counts, sums = _report(z, p, np.ones((H, W), np.uint8), np.ones((H, W), np.uint8))
    assert counts.tolist() == _closed_counts(H, W, 0, H, 0, W)
    assert d["scales"][0]["fill_rms"] == 4 * a and sums[0].tolist() == [0.0, counts[0] * 16 * a * a, 0.0]
    for s in d["scales"][1:]:
        assert s["fill_rms"] == 0.0, s
    assert (sums[1:] == 0).all()


def test_identity():
    rng = np.random.default_rng(3)
    H, W = 45, 70
    z = rng.integers(-1000, 1001, (H, W)).astype(np.float32)
    sel = np.zeros((H, W), np.uint8)
    sel[3:40, 10:66] = 1
    d, counts, sums = _report(z, z.copy(), sel, np.ones((H, W), np.uint8))
    assert d["scales_scored"] == 10 and d["log_ratio_rms"] == 0.0
    for s, row in zip(d["scales"], sums):
        assert row[0] > 0 and row[0] == row[1] == row[2]
        assert s["ratio"] == 1.0 and s["corr"] == 1.0 and s["truth_rms"] == s["fill_rms"] > 0


def test_arms_off_the_raster_or_unknown():
    one = lambda H, W: np.ones((H, W), np.uint8)
    rng = np.random.default_rng(4)
    # an unknown pixel drops the triple it centres and the two it is an arm of, per direction
    z = rng.integers(-9, 10, (9, 9)).astype(np.float32)
    known = one(9, 9)
    known[4, 4] = 0
    counts, sums, _ = TO.spectrum(z, z, one(9, 9), known, 1)
    assert counts.tolist() == [2 * (9 * 7 - 3), 2 * (7 * 7 - 3)] + [0] * 8
    zn = z.copy()
    zn[4, 4] = np.nan                                    # never read into a sum
    assert np.array_equal(TO.spectrum(zn, zn, one(9, 9), known, 1)[1], sums)
    # sel restricts the centres, not the arms
    sel = np.zeros((9, 9), np.uint8)
    sel[0, 0] = sel[2, 2] = 1
    assert TO.spectrum(z, z, sel, one(9, 9), 2)[0].tolist() == [2, 2, 2, 2] + [0] * 6
    # sides shorter than 2 h + 1: the steps that need that side have no triple
    for H, W in ((1, 1), (1, 40), (3, 3), (3, 40), (4, 4), (40, 1), (33, 33), (32, 33)):
        z = rng.integers(-9, 10, (H, W)).astype(np.float32)
        d, counts, sums = _report(z, z, one(H, W), one(H, W))
        assert counts.tolist() == _closed_counts(H, W, 0, H, 0, W), (H, W)
        for j in range(5):
            h = 1 << j
            ax, dg = d["scales"][2 * j], d["scales"][2 * j + 1]
            assert ax["triples"] == H * max(0, W - 2 * h) + max(0, H - 2 * h) * W
            assert dg["triples"] == 2 * max(0, H - 2 * h) * max(0, W - 2 * h)
            if max(H, W) < 2 * h + 1:
                assert ax["triples"] == 0
            if min(H, W) < 2 * h + 1:
                assert dg["triples"] == 0
            for s in (ax, dg):
                if s["triples"] == 0:
                    assert s["truth_rms"] is None and s["fill_rms"] is None and s["ratio"] is None and s["corr"] is None
    d, counts, _ = _report(np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32), one(1, 1), one(1, 1))
    assert counts.tolist() == [0] * 10 and d["scales_scored"] == 0 and d["log_ratio_rms"] is None
    d, counts, _ = _report(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), one(3, 3), one(3, 3))
    assert counts.tolist() == [6, 2] + [0] * 8


def test_octaves_not_requested_are_zero():
    rng = np.random.default_rng(6)
    z = rng.integers(-50, 51, (40, 40)).astype(np.float32)
    p = rng.integers(-50, 51, (40, 40)).astype(np.float32)
    full = TO.spectrum(z, p, np.ones((40, 40)), np.ones((40, 40)), 5)
    for o in (1, 3):
        counts, sums, asum = TO.spectrum(z, p, np.ones((40, 40)), np.ones((40, 40)), o)
        assert np.array_equal(counts[:2 * o], full[0][:2 * o]) and np.array_equal(sums[:2 * o], full[1][:2 * o])
        assert (counts[2 * o:] == 0).all() and (sums[2 * o:] == 0).all() and (asum[2 * o:] == 0).all()
        assert (asum[:2 * o, :2] == sums[:2 * o, :2]).all() and (asum[:, 2] >= np.abs(sums[:, 2])).all()


# ---- the pure halves of the row ------------------------------------------------------------------------------------------
def test_assemble_texture():
    from mvp_gan.src.evaluate_raster import assemble_texture, texture_summary
    counts = [4, 2, 8, 0, 3, 5, 0, 0, 9, 9]
    sums = [[16.0, 64.0, 24.0],      # truth_rms 2, fill_rms 4, ratio 2, corr 24 / 32
            [8.0, 2.0, -4.0],        # truth_rms 2, fill_rms 1, ratio 0.5, corr -1
            [0.0, 32.0, 0.0],        # Szz == 0: no ratio, no corr
            [0.0, 0.0, 0.0],         # n == 0
            [27.0, 0.0, 0.0],        # Spp == 0: ratio 0, no corr, not scored
            [5.0, 5.0, 5.0],
            [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    d = assemble_texture(counts, sums, cellsize=2.0, octaves=3)
    assert list(d) == ["octaves", "scales", "scales_scored", "log_ratio_rms"] and d["octaves"] == 3 and len(d["scales"]) == 6
    assert [(s["lag_px"], s["class"]) for s in d["scales"]] == [(1, "axial"), (1, "diagonal"), (2, "axial"), (2, "diagonal"),
                                                                (4, "axial"), (4, "diagonal")]
    lags = [s["lag_m"] for s in d["scales"]]
    assert lags == sorted(lags) and lags[0] == 2.0 and lags[1] == 2.0 * math.sqrt(2.0) and lags[4] == 8.0
    assert [s["triples"] for s in d["scales"]] == counts[:6]
    keys = ["lag_px", "class", "lag_m", "triples", "truth_rms", "fill_rms", "ratio", "corr"]
    assert all(list(s) == keys for s in d["scales"])
    s0, s1, s2, s3, s4, s5 = d["scales"]
    assert (s0["truth_rms"], s0["fill_rms"], s0["ratio"], s0["corr"]) == (2.0, 4.0, 2.0, 0.75)
    assert (s1["truth_rms"], s1["fill_rms"], s1["ratio"], s1["corr"]) == (2.0, 1.0, 0.5, -1.0)
    assert (s2["truth_rms"], s2["fill_rms"], s2["ratio"], s2["corr"]) == (0.0, 2.0, None, None)
    assert (s3["truth_rms"], s3["fill_rms"], s3["ratio"], s3["corr"]) == (None, None, None, None)
    assert (s4["truth_rms"], s4["fill_rms"], s4["ratio"], s4["corr"]) == (3.0, 0.0, 0.0, None)
    assert (s5["truth_rms"], s5["fill_rms"], s5["ratio"], s5["corr"]) == (1.0, 1.0, 1.0, 1.0)
    assert d["scales_scored"] == 3
    assert d["log_ratio_rms"] == math.sqrt((math.log(2.0) ** 2 + math.log(0.5) ** 2 + 0.0) / 3)
    txt = json.dumps(d)
    assert "NaN" not in txt and json.loads(txt) == d
    line = texture_summary(d)
    assert line.startswith("texture:") and "1 px axial ratio 2.000 corr 0.750" in line and "4 px diagonal ratio 1.000 corr 1.000" in line
    assert "n/a" not in line and "3 of 6 scales" in line and "\n" not in line
    # numpy inputs, as the tests hand them over
    assert assemble_texture(np.array(counts), np.array(sums), cellsize=np.float32(2.0), octaves=np.int64(3)) == d
    none = assemble_texture([0] * 10, [[0.0] * 3] * 10, cellsize=1.0, octaves=5)
    assert none["scales_scored"] == 0 and none["log_ratio_rms"] is None and len(none["scales"]) == 10
    assert all(s["truth_rms"] is None and s["corr"] is None for s in none["scales"])
    line = texture_summary(none)
    assert "n/a" in line and "0 of 10 scales" in line and json.loads(json.dumps(none)) == none
    with pytest.raises(ValueError, match="octaves"):
        assemble_texture(counts, sums, cellsize=1.0, octaves=6)
    with pytest.raises(ValueError, match="cellsize"):
        assemble_texture(counts, sums, cellsize=0.0, octaves=5)


def test_texture_row_assembly():
    """The place of the row in assemble_compare, and the signatures."""
    from mvp_gan.src import evaluate_raster as ER
    raw = {"idw": {"height": 1}, "nearest": {"height": 2}}
    infos = {"idw": {"a": 1}, "nearest": {"a": 2}}
    cmp = ER.assemble_compare(raw, infos)
    assert all("texture" not in cmp[k] and set(cmp[k]) == {"height", "method", "fill"} for k in cmp)
    a, b = {"octaves": 1}, {"octaves": 2}
    cmp = ER.assemble_compare(raw, infos, None, None, None, None, {"idw": a, "nearest": b})
    assert cmp["idw"]["texture"] is a and cmp["nearest"]["texture"] is b and "wetness" not in cmp["idw"] and "texture" not in raw["idw"]
    cmp = ER.assemble_compare(raw, infos, texture={"idw": a, "nearest": b}, wetness={"idw": b, "nearest": a})
    assert cmp["idw"]["texture"] is a and cmp["idw"]["wetness"] is b
    assert list(inspect.signature(ER.assemble_compare).parameters)[-1] == "texture"
    for fn in (ER.texture_errors, ER.texture_raw):
        sig = inspect.signature(fn).parameters
        assert [(k, sig[k].default) for k in list(sig)[3:]] == [("cellsize", inspect.Parameter.empty), ("mask", None), ("nodata", None),
                                                                ("octaves", 5)]
    for fn in (ER.evaluate_raster, ER.baseline_report, ER.compare_report):
        sig = inspect.signature(fn).parameters
        assert (sig["texture"].default, sig["texture_octaves"].default) == (False, 5)
        assert sig["texture"].kind == sig["texture_octaves"].kind == inspect.Parameter.KEYWORD_ONLY
    from mvp_gan.src.texture import texture_spectrum
    sig = inspect.signature(texture_spectrum).parameters
    assert [(k, sig[k].default) for k in sig] == [("dem", inspect.Parameter.empty), ("mask", None), ("nodata", None), ("cellsize", 1.0),
                                                  ("octaves", 5), ("where", None)]


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_check_octaves():
    from mvp_gan.src.evaluate_raster import check_octaves, texture_errors
    from mvp_gan.src.texture import texture_spectrum
    for good in (1, 5, np.int64(3), np.int32(2), np.uint8(4)):
        assert check_octaves(good, "t") == int(good) and type(check_octaves(good, "t")) is int
    z = np.zeros((4, 4), np.float32)
    for bad in (0, 6, -1, 1.5, 2.0, True, False, np.bool_(True), np.float64(3.0), "3", None):
        with pytest.raises(ValueError, match="octaves"):
            check_octaves(bad, "t")
        with pytest.raises(ValueError, match="octaves"):
            texture_errors(z, z, z, cellsize=1.0, octaves=bad)
        with pytest.raises(ValueError, match="octaves"):
            texture_spectrum(z, octaves=bad)
    with pytest.raises(ValueError, match="who: octaves"):
        check_octaves(0, "who")
    # shapes and the cell size are refused on the host too
    with pytest.raises(ValueError, match="pred"):
        texture_errors(z, np.zeros((4, 5), np.float32), z, cellsize=1.0)
    with pytest.raises(ValueError, match="holes"):
        texture_errors(z, z, np.zeros((3, 4), np.uint8), cellsize=1.0)
    with pytest.raises(ValueError, match="cellsize"):
        texture_errors(z, z, z, cellsize=0.0)
    with pytest.raises(ValueError, match="where"):
        texture_spectrum(z, where=np.zeros((4, 5), np.uint8))
    with pytest.raises(ValueError, match="cellsize"):
        texture_spectrum(z, cellsize=-1.0)


def test_c_entry_points_reject_without_gpu():
    import ctypes as C
    import __graft_entry__ as ge
    ge.build()
    from tg_hip import lib as L
    lib = L.load()
    assert (L.TG_TEX_OCTAVES, L.TG_TEX_SCALES, L.TG_TEX_NSUM) == (TO.OCTAVES, TO.SCALES, TO.NSUM)
    assert lib.tg_texture_ws_bytes(0, 5) == 0 and lib.tg_texture_ws_bytes(5, 0) == 0 and lib.tg_texture_ws_bytes(-1, 5) == 0
    assert lib.tg_texture_ws_bytes(1 << 16, 1 << 15) == 0
    # one row of 10 x 3 doubles per workgroup, a workgroup per 32 x 64 tile up to 2048
    row = 10 * 3 * 8
    for H, W in [(1, 1), (32, 64), (33, 64), (32, 65), (97, 130), (200, 300), (8192, 8192), (1, (1 << 31) - 1), (46340, 46340)]:
        tiles = -(-H // 32) * -(-W // 64)
        assert lib.tg_texture_ws_bytes(H, W) == min(tiles, 2048) * row > 0, (H, W)
    one = C.c_void_p(8)                                                  # non-null, never dereferenced: every call is refused
    need = lib.tg_texture_ws_bytes(4, 4)
    args = lambda **kw: [kw.get(k, one) for k in ("z", "p", "sel", "known")] + [kw.get("H", 4), kw.get("W", 4), kw.get("octaves", 5)] + \
        [kw.get(k, one) for k in ("counts", "sums", "ws")] + [kw.get("ws_bytes", need), None]
    for name in ("z", "p", "sel", "known", "counts", "sums", "ws"):
        assert lib.tg_texture_compare(*args(**{name: None})) == -1
        msg = lib.tg_last_error()
        assert b"tg_texture_compare" in msg and b"null pointer " + name.encode() in msg, msg
    for kw in ({"H": 0}, {"W": 0}, {"H": 1 << 16, "W": 1 << 15}):
        assert lib.tg_texture_compare(*args(**kw)) == -1 and b"raster" in lib.tg_last_error()
    for o in (0, 6, -1):
        assert lib.tg_texture_compare(*args(octaves=o)) == -1 and b"octaves" in lib.tg_last_error()
    assert lib.tg_texture_compare(*args(ws_bytes=need - 1)) == -1 and b"ws_bytes" in lib.tg_last_error()
    assert lib.tg_texture_compare(*args(ws_bytes=0)) == -1 and b"ws_bytes" in lib.tg_last_error()


# ---- parsers -------------------------------------------------------------------------------------------------------------
def test_cli_parsers():
    from mvp_gan.src.evaluate_raster import build_parser
    base = ["--dem", "x.asc", "--pred", "p.asc", "--holes", "h.png"]
    a = build_parser().parse_args(base + ["--texture", "--octaves", "3"])
    assert a.texture is True and a.octaves == 3
    a = build_parser().parse_args(base)
    assert a.texture is False and a.octaves == 5 and not a.wetness
    a = build_parser().parse_args(["--dem", "x.asc", "--checkpoint", "c.pth", "--texture"])
    assert a.texture and a.octaves == 5
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--octaves", "1.5"])
    from mvp_gan.src import evaluate_raster as ER
    for bad in ("0", "6"):
        with pytest.raises(SystemExit):
            ER.main(base + ["--texture", "--octaves", bad])            # refused before any file is opened
    from mvp_gan.src import texture as T
    a = T.build_parser().parse_args(["--dem", "in.asc"])
    assert (a.dem, a.mask, a.nodata, a.octaves, a.json) == ("in.asc", None, None, 5, None)
    a = T.build_parser().parse_args(["--dem", "in.asc", "--mask", "m.png", "--nodata", "-9999", "--octaves", "2", "--json", "o.json"])
    assert (a.mask, a.nodata, a.octaves, a.json) == ("m.png", -9999.0, 2, "o.json")
    for bad in (["--octaves", "0"], ["--octaves", "6"]):
        with pytest.raises(SystemExit):
            T.main(["--dem", "in.asc"] + bad)
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--octaves", "2"])               # --dem is required
